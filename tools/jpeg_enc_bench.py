"""GPU JPEG writer at 1080p (csrc/jpeg_enc.hip, DESIGN.md §6, `--jpeg_writer gpu`): HIP-event time of one
nst_jpeg_encode_u8 call over a batch of 8 frames (median of the timed calls after warm-up) at quality 85 and 95, on
stylized frames (the model's output for the bench's synthetic frames) and on noise; the mean file size; one
byte-for-byte check of every file against Pillow.

The per-launch split comes from a kernel trace of a second, short run of this tool:
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o run -- python tools/jpeg_enc_bench.py --iters 5
  python tools/jpeg_enc_bench.py --kernel-stats DIR/.../run_kernel_stats.csv [--forward-ms MS] [--out FILE]
(--forward-ms: bench.py's ms_per_step of the same session, put beside the encode time).
"""
from __future__ import annotations

import argparse
import csv
import io
import json
import os
import statistics
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np
from PIL import Image

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def _pil(frame, q):
    b = io.BytesIO()
    Image.fromarray(frame).save(b, format="JPEG", quality=q)
    return b.getvalue()


def _kernel_split(path):
    """rocprofv3's kernel stats -> {kernel: {calls, avg_us, share of the encoder's kernel time}} for the encoder"""
    rows = [r for r in csv.DictReader(open(path)) if "jpeg_enc" in r["Name"]]
    total = sum(float(r["TotalDurationNs"]) for r in rows) or 1.0
    out = {}
    for r in rows:
        name = r["Name"].split("jpeg_enc_")[-1].split("(")[0]
        name = "jpeg_enc_" + ("scan_chunks" if "<true>" in r["Name"] else "scan_blocks" if "<false>" in r["Name"] else name)
        out[name] = {"calls": int(r["Calls"]), "avg_us": round(float(r["AverageNs"]) / 1e3, 2),
                     "share": round(float(r["TotalDurationNs"]) / total, 4)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--threads", type=int, default=min(16, os.cpu_count() or 1))
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--kernel-stats", default=None, help="rocprofv3 kernel stats CSV of a traced run of this tool")
    ap.add_argument("--forward-ms", type=float, default=None, help="bench.py ms_per_step of the same session")
    ap.add_argument("--forward-batch", type=int, default=None, help="frames per bench.py step")
    ap.add_argument("--out", default=None, help="also write the JSON here")
    args = ap.parse_args()
    import torch

    from neuralstyletransferv1_amd import jpegio, synthetic
    from neuralstyletransferv1_amd.transformer_net import TransformerNet

    h, w = 1080, 1920
    dev = torch.device("cuda", 0)
    net = TransformerNet()
    net.load_state_dict(synthetic.make_state_dict("johnson", 0))
    net = net.to(dev).eval()
    net.compute_dtype = "bf16"
    src = torch.from_numpy(synthetic.make_frames(args.batch, h, w, seed=300)).to(dev)
    stylized = net.engine(dev).stylize_u8(src, "imagenet_255")
    noise = torch.from_numpy(np.random.default_rng(7).integers(0, 256, (args.batch, h, w, 3), dtype=np.uint8)).to(dev)
    res = {"frame_hw": [h, w], "batch": args.batch, "iters": args.iters, "bound_bytes": jpegio.jpeg_enc_bound(h, w),
           "workspace_bytes": jpegio.jpeg_enc_workspace_bytes(args.batch, h, w), "threads": args.threads}
    pool = ThreadPoolExecutor(args.threads)
    for name, x in (("stylized", stylized), ("noise", noise)):
        host = x.cpu().numpy()
        for q in (85, 95):
            files, sizes = jpegio.encode_jpeg_gpu(x, q)
            sz = sizes.cpu().tolist()
            fh = files.cpu().numpy()
            want = list(pool.map(lambda f: _pil(f, q), host))
            exact = all(fh[j, :sz[j]].tobytes() == want[j] for j in range(args.batch))
            ts = []
            for it in range(args.iters + 3):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                jpegio.encode_jpeg_gpu(x, q)
                e1.record()
                torch.cuda.synchronize()
                if it >= 3:
                    ts.append(e0.elapsed_time(e1))
            med = statistics.median(ts)
            row = {"bytes_equal_pillow": bool(exact), "encode_ms_median": round(med, 4),
                   "encode_ms_min": round(min(ts), 4), "encode_ms_max": round(max(ts), 4),
                   "gpu_frames_per_s": round(args.batch / med * 1e3, 1),
                   "mean_file_bytes": int(np.mean(sz)), "max_file_bytes": int(max(sz)),
                   "fits_pixel_slot": bool(max(sz) <= h * w * 3)}
            res[f"{name}_q{q}"] = row
            print(f"{name} q{q}", json.dumps(row), flush=True)
            assert exact, f"{name} q{q}: the files differ from Pillow's"
    if args.kernel_stats:
        res["per_launch"] = _kernel_split(args.kernel_stats)
    if args.forward_ms is not None:
        res["forward_ms_per_step"] = args.forward_ms
        res["forward_batch"] = args.forward_batch
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
