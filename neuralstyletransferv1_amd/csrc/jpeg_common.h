// Geometry and record layout shared by the host entropy decoder (jpeg_entropy.cpp) and the reconstruction kernels
// (jpeg_dec.hip).  Plain C++: no HIP, so the entropy decoder builds stand-alone (tools/asan/jpeg_entropy_asan.cpp).
//
// One frame's coefficient record:
//   uint16 qt[3][64]      dequantisation table of component 0..2 in natural (row-major) order (unused ones zero)
//   int16  coef[blocks][64]  quantised coefficients in natural order, planar by component: component c's blocks
//                         start at block blk_off[c], bw[c] x bh[c] of them in raster order (the MCU grid's padding
//                         blocks included, as the scan codes them)
// The planar u8 workspace of the kernels mirrors it: 64 bytes per block, plane c at byte blk_off[c]*64 with a row
// pitch of bw[c]*8.
#pragma once
#include <stddef.h>
#include <stdint.h>

#define NST_JPEG_QT_BYTES 384  // 3 tables x 64 x uint16

struct JpegGeom {
  int comps, hs, vs;  // components (1 or 3); luma sampling factors (chroma is 1x1)
  int bw[3], bh[3];   // blocks per plane as coded
  int pw[3], ph[3];   // real samples per plane: ceil(w*hs_c/hmax), ceil(h*vs_c/vmax)
  size_t blk_off[3];  // first block of each plane
  size_t blocks;      // blocks per frame
};

// sampling: 0 = 4:4:4 (and every single-component image), 1 = 4:2:2 (h2v1), 2 = 4:2:0 (h2v2)
static inline bool jpeg_geom(int h, int w, int comps, int sampling, JpegGeom* g) {
  if (h <= 0 || w <= 0 || h > 65535 || w > 65535 || (comps != 1 && comps != 3) || sampling < 0 || sampling > 2 ||
      (comps == 1 && sampling != 0))
    return false;
  g->comps = comps;
  g->hs = sampling >= 1 ? 2 : 1;
  g->vs = sampling == 2 ? 2 : 1;
  const int mcux = (w + 8 * g->hs - 1) / (8 * g->hs), mcuy = (h + 8 * g->vs - 1) / (8 * g->vs);
  size_t off = 0;
  for (int c = 0; c < 3; ++c) {
    g->blk_off[c] = off;
    if (c >= comps) {
      g->bw[c] = g->bh[c] = g->pw[c] = g->ph[c] = 0;
      continue;
    }
    g->bw[c] = c == 0 ? mcux * g->hs : mcux;
    g->bh[c] = c == 0 ? mcuy * g->vs : mcuy;
    g->pw[c] = c == 0 ? w : (w + g->hs - 1) / g->hs;
    g->ph[c] = c == 0 ? h : (h + g->vs - 1) / g->vs;
    off += (size_t)g->bw[c] * g->bh[c];
  }
  g->blocks = off;
  return true;
}

static inline size_t jpeg_record_bytes(const JpegGeom& g) { return NST_JPEG_QT_BYTES + g.blocks * 128; }
