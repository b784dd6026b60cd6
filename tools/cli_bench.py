"""End-to-end CLI frames/s at 1080p on one GPU: the reference's frame paths
through this engine's pipeline, for PNG and JPEG frames, beside the host decode / encode rates alone (the same
thread count), so the host I/O share of the wall time is measured, not assumed.

Two paths per format:
  * "input_dir": pipeline.main --input_dir (image batch mode, pipeline.py:2575-2606): each source is staged (EXIF
    upright, JPEG re-encoded at --jpeg_quality, in memory here), stylized, LAB-smoothed, blended and saved.
    A JPEG frame costs four host codec operations (decode, staging encode + decode, output encode).
  * "frames_dir": the video path's per-frame loop after ffmpeg has extracted the frames (pipeline.py:1080-2119:
    decode -> stylize -> LAB EMA -> blend -> encode), run on a directory of frame_*.{png,jpg} files.

Default CLI settings (bf16, --batch 8, --blend 0.9, --smooth_alpha 0.65, staged/output JPEG at the default
--jpeg_quality 85 from quality-95 source files, PNG through the default fast writer) on synthetic frames (smooth gradients + shapes + ~5 LSB
noise, neuralstyletransferv1_amd/synthetic.py).  The timed run excludes the model load (a warm-up run first).

  python tools/cli_bench.py [--frames 240] [--threads 16] [--png_writer fast|pil|gpu] [--jpeg_reader pil|gpu]
      [--jpeg_writer pil|gpu]
"""
from __future__ import annotations

import argparse
import json
import os
import shutil
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

import numpy as np
import torch
from PIL import Image

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def _run_ranks(P, args, vargv, fd, ck, ext, tmp):
    """The frames_dir loop as `--gpus N --dist_backend gloo` (pipeline._worker per rank, as pipeline.main spawns
    them): every rank decodes, stylizes and encodes its own round-robin shard; rank 0 runs the ordered LAB EMA
    over the L planes.  -> (frames written, wall seconds, per-rank record)."""
    import socket

    import torch.multiprocessing as mp
    wdir = os.path.join(tmp, f"written_{ext}")
    os.makedirs(wdir, exist_ok=True)
    os.environ["NST_PIPE_WRITTEN"] = wdir
    thr = max(1, args.threads // args.gpus)
    argv = [a for a in vargv] + ["--dist_backend", "gloo", "--dist_timeout", "300", "--model_type", "transformer"]
    i = argv.index("--threads")
    argv[i + 1] = str(thr)
    prep = (fd, Path(ck), {}, False, True)
    out = None
    for rep in range(2):  # warm-up, then timed
        with socket.socket() as s:
            s.bind(("127.0.0.1", 0))
            port = s.getsockname()[1]
        t0 = time.perf_counter()
        mp.start_processes(P._worker, args=(args.gpus, argv, port, prep, None), nprocs=args.gpus, start_method="spawn")
        t_cli = time.perf_counter() - t0
        out = t_cli
    del os.environ["NST_PIPE_WRITTEN"]
    ranks = {}
    n = 0
    for r in range(args.gpus):
        d = json.load(open(os.path.join(wdir, f"rank{r}.json")))
        n += len(d["written"])
        ranks[f"rank{r}"] = {"frames": len(d["written"]), "loop_s": round(d["loop_seconds"], 3),
                             "loop_frames_per_s": round(len(d["written"]) / d["loop_seconds"], 2),
                             "setup_s": round(d["setup_seconds"], 3)}
    ranks.update({"ranks": args.gpus, "threads_per_rank": thr, "wall_s_incl_spawn": round(out, 3),
                  "job_loop_frames_per_s": round(n / max(v["loop_s"] for k, v in ranks.items() if k.startswith("rank")), 2),
                  "note": "gloo, every rank on GPU 0 of one box (a rehearsal of the orchestration, not a scaling run)"})
    return n, out, ranks


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=240)
    ap.add_argument("--threads", type=int, default=int(os.environ.get("OMP_NUM_THREADS", "16") or 16))
    ap.add_argument("--png_writer", default="fast", choices=["fast", "pil", "gpu"],
                    help="the CLI's PNG writer; the host-only encode rate beside it uses pngio's writer for fast/gpu")
    ap.add_argument("--jpeg_reader", default="pil", choices=["pil", "gpu"],
                    help="the CLI's JPEG frame reader (frames_dir path; --input_dir staging always decodes with Pillow)")
    ap.add_argument("--jpeg_writer", default="pil", choices=["pil", "gpu"], help="the CLI's JPEG writer")
    ap.add_argument("--formats", default="jpg,png")
    ap.add_argument("--paths", default="frames_dir,input_dir")
    ap.add_argument("--gpus", type=int, default=1,
                    help="frames_dir path only: N ranks (--dist_backend gloo, every rank on GPU 0 of this box, "
                         "--threads split between them): the multi-GPU orchestration with each rank encoding its "
                         "own frames; per-rank frames/s reported")
    args = ap.parse_args()
    from neuralstyletransferv1_amd import pipeline as P
    from neuralstyletransferv1_amd import pngio, synthetic

    tmp = tempfile.mkdtemp(prefix="nst_cli_")
    ck = os.path.join(tmp, "johnson.pth")
    torch.save(synthetic.make_state_dict("johnson", 0), ck)
    frames = synthetic.make_frames(8, 1080, 1920, seed=300)
    res = {"frames": args.frames, "threads": args.threads, "frame_hw": [1080, 1920], "png_writer": args.png_writer,
           "jpeg_reader": args.jpeg_reader, "jpeg_writer": args.jpeg_writer,
           "data": "synthetic 1080p frames (8 distinct, cycled)"}
    pool = ThreadPoolExecutor(args.threads)
    for ext in args.formats.split(","):
        d_in = os.path.join(tmp, f"in_{ext}")
        os.makedirs(d_in)
        paths = [os.path.join(d_in, f"frame_{i + 1:04d}.{ext}") for i in range(args.frames)]

        def enc_in(i):
            if ext == "png":
                pngio.write_png(paths[i], frames[i % len(frames)])
            else:
                Image.fromarray(frames[i % len(frames)]).save(paths[i], format="JPEG", quality=95)
        list(pool.map(enc_in, range(args.frames)))
        host = {}
        t0 = time.perf_counter()
        list(pool.map(lambda p: np.asarray(Image.open(p).convert("RGB")), paths))
        host["host_decode_frames_per_s"] = round(args.frames / (time.perf_counter() - t0), 1)
        d_enc = os.path.join(tmp, f"enc_{ext}")
        os.makedirs(d_enc)

        def enc_out(i):
            p = os.path.join(d_enc, f"o_{i:04d}.{ext}")
            if ext == "jpg":
                Image.fromarray(frames[i % len(frames)]).save(p, format="JPEG", quality=95)
            elif args.png_writer in ("fast", "gpu"):
                pngio.write_png(p, frames[i % len(frames)])
            else:
                Image.fromarray(frames[i % len(frames)]).save(p)
        t0 = time.perf_counter()
        list(pool.map(enc_out, range(args.frames)))
        host["host_encode_frames_per_s"] = round(args.frames / (time.perf_counter() - t0), 1)
        shutil.rmtree(d_enc)
        res[ext] = dict(host)
        common = ["--model", ck, "--io_preset", "imagenet_255", "--dtype", "bf16", "--batch", "8", "--blend", "0.9",
                  "--smooth_alpha", "0.65", "--image_ext", ext, "--threads", str(args.threads),
                  "--png_writer", args.png_writer, "--jpeg_reader", args.jpeg_reader,
                  "--jpeg_writer", args.jpeg_writer]
        for path in args.paths.split(","):
            if path == "input_dir":
                d_out = os.path.join(tmp, f"out_{ext}")
                argv = ["--input_dir", d_in, "--output_dir", d_out, "--work_dir", os.path.join(tmp, f"w_{ext}")] + common
                P.main(argv[:4] + ["--max_frames", "8"] + argv[4:])  # warm-up: model load, kernels, LAB tables
                t0 = time.perf_counter()
                rc = P.main(argv)
                t_cli = time.perf_counter() - t0
                assert rc == 0
                n_out = len(list(Path(d_out).glob(f"*.{ext}")))
            else:
                # the video path after extraction: style_frames over work_dir/frames (frame_*.ext), outputs
                # styled_frame_*.ext beside them (pipeline.py:1080-2119)
                wd = Path(tmp) / f"v_{ext}"
                fd = wd / "frames"
                fd.mkdir(parents=True)
                for p in paths:
                    os.link(p, fd / os.path.basename(p))
                vargv = ["--input_video", "x", "--output_video", "y", "--work_dir", str(wd)] + common
                if args.gpus > 1:
                    n_out, t_cli, ranks = _run_ranks(P, args, vargv, fd, ck, ext, tmp)
                    res[ext][path + f"_gpus{args.gpus}"] = ranks
                    print(ext, path, args.gpus, json.dumps(ranks), flush=True)
                    continue
                a = P.build_parser().parse_args(vargv)
                a.model_type = "transformer"
                P._run_style(a, fd, Path(ck), {}, False)  # warm-up (writes the outputs once)
                t0 = time.perf_counter()
                P._run_style(a, fd, Path(ck), {}, False)
                t_cli = time.perf_counter() - t0
                n_out = len(list(fd.glob(f"styled_frame_*.{ext}")))
            assert n_out == args.frames, (path, n_out)
            st = dict(P.LAST_RUN_STATS)
            # wall time of the whole call (model load and plans included), and the frame loop's own rate
            res[ext][path] = {"cli_frames_per_s": round(args.frames / t_cli, 2), "cli_s": round(t_cli, 3),
                              "loop_frames_per_s": round(st["frames"] / st["seconds"], 2),
                              "setup_s": round(st["setup_seconds"], 3)}
            print(ext, path, json.dumps(res[ext][path]), flush=True)
        shutil.rmtree(d_in)
    shutil.rmtree(tmp, ignore_errors=True)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
