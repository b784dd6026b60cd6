// conv_launch.h — host side shared by the conv launchers: the device's CU count, the persistent grid, the
// frames-per-launch loop and the common head of a ConvKernelInfo.  No device code (the variant ladders, which pick a
// kernel instantiation, stay with their kernels).
#pragma once
#include <algorithm>
#include <cstring>

#include "nst_internal.h"

namespace nst {

// CUs of the current device, queried once per process (256 if the query fails).  One value for every launcher and
// device: all GPUs of a box are the same part, so it is what each launcher's own first query returned.
inline int device_cus() {
  static const int v = [] {
    int dev = 0, c = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&c, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess)
      c = 256;
    return c;
  }();
  return v;
}

// Grid of a persistent launch: n_work work items walked by at most `resident` workgroups (the kernel's resident
// workgroups on the device), under the grid cap; reports the launch to the op record being run.
inline int persistent_grid(int n_work, int resident) {
  const int nb = capped_blocks(std::min(n_work, resident));
  note_launch(nb, n_work);
  return nb;
}

// Frames-per-launch loop of the kernels that hold their frames' InstanceNorm tables in LDS: n frames of ntile work
// items each, in chunks of at most min(nfmax, byte_frames) frames (nfmax: the LDS tables' capacity; byte_frames: the
// frames the kernel's 32-bit buffer offsets reach).  Each chunk gets its own ConvParams with every per-frame pointer
// that is set advanced to the chunk's first frame, n_work and the persistent grid of `resident` workgroups, and goes
// to the kernel's variant dispatch go(p, nb).  res_r and res_out share the input's layout; the InstanceNorm partials
// are part_rows rows per tile.
template <typename Go>
void launch_frame_chunks(const ConvParams& p0, int ntile, int n, size_t nfmax, size_t byte_frames, int part_rows,
                         int resident, Go go) {
  const size_t fin = (size_t)p0.hs * p0.ws * p0.cs * 2, fout = (size_t)p0.oh * p0.ow * p0.cout_stride * 2;
  const int fmax = (int)std::min(nfmax, byte_frames);
  if (fmax < 1) return;  // nst_api validates sizes before launching
  for (int f0 = 0; f0 < n; f0 += fmax) {
    ConvParams p = p0;
    p.in = (const char*)p0.in + f0 * fin;
    p.out = (char*)p0.out + f0 * fout;
    if (p0.res_r) p.res_r = (const char*)p0.res_r + f0 * fin;
    if (p0.res_out) p.res_out = (char*)p0.res_out + f0 * fin;
    if (p0.in_norm) p.in_norm = p0.in_norm + (size_t)f0 * p0.cs;
    if (p0.res_rnorm) p.res_rnorm = p0.res_rnorm + (size_t)f0 * p0.cs;
    if (p0.partial) p.partial = p0.partial + (size_t)f0 * ntile * part_rows * p0.cout_stride * 2;
    p.n_work = std::min(fmax, n - f0) * ntile;
    go(p, persistent_grid(p.n_work, resident));
  }
}

// Common head of a kernel's ConvKernelInfo: every field zero but the dtype, the mode, activation input and output,
// one InstanceNorm partial row per tile, the persistent flag and the launcher.  A kernel's info() sets what is its own.
inline ConvKernelInfo conv_info(int dtype, int mode, void (*launch)(const ConvParams&, dim3, hipStream_t),
                                bool persistent = true) {
  ConvKernelInfo k;
  std::memset(&k, 0, sizeof(k));
  k.dtype = dtype;
  k.mode = mode;
  k.in_kind = IN_ACT; k.out_kind = OUT_ACT;
  k.persistent = persistent ? 1 : 0;
  k.part_rows = 1;
  k.launch = launch;
  return k;
}

}  // namespace nst
