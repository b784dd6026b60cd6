// Host half of the baseline JPEG reader (--jpeg_reader gpu): marker parse, byte unstuffing, Huffman decode, DC
// prediction and de-zigzag of one frame into its coefficient record (jpeg_common.h); the reconstruction runs on the
// device (jpeg_dec.hip).  Plain C++: no HIP call, no global state, safe to call from many threads at once.
//
// The fast path is deliberately narrow (SOF0, one scan holding every component, 8-bit tables, JFIF YCbCr at
// 4:4:4 / 4:2:2 / 4:2:0 or a single component, optional restart intervals) and takes clean streams only: anything
// else returns NST_E_SHAPE (a stream this decoder does not take) or NST_E_DATA (a damaged one) and the caller hands
// the file to Pillow, which then warns, raises or decodes as it always did.
#include <string.h>

#include <string>

#include "jpeg_common.h"
#include "nst_hip.h"

namespace nst {
void set_error(const std::string& msg);  // nst_api.cpp (the stand-alone sanitizer program brings its own)
}
using nst::set_error;

namespace {

const uint8_t kZigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                             41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                             30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

constexpr int kLook = 9;

struct HuffTable {
  bool defined = false;
  uint16_t look[1 << kLook];  // (code length << 8) | symbol for codes of <= kLook bits, 0 otherwise
  int32_t maxcode[18];        // largest code of each length, -1 where the length has none
  int32_t valoff[17];         // index of a length's first symbol minus its first code
  uint8_t vals[256];
};

struct Header {
  int h = 0, w = 0, comps = 0, sampling = 0;
  int tq[3] = {0, 0, 0}, td[3] = {0, 0, 0}, ta[3] = {0, 0, 0};
  bool qt_defined[4] = {false, false, false, false};
  uint16_t qt[4][64];  // natural order
  HuffTable dc[4], ac[4];
  int restart = 0;
  size_t scan_pos = 0;  // first byte of the entropy-coded segment
  JpegGeom geom;
};

// canonical code construction (ITU T.81 Annex C), refusing over-subscribed lengths
bool build_table(HuffTable& t, const uint8_t* counts, const uint8_t* syms, int nsyms) {
  memset(t.look, 0, sizeof(t.look));
  memcpy(t.vals, syms, nsyms);
  memset(t.vals + nsyms, 0, 256 - nsyms);
  int code = 0, k = 0;
  for (int l = 1; l <= 16; ++l) {
    const int cnt = counts[l - 1];
    t.valoff[l] = k - code;
    if (cnt) {
      if (code + cnt > (1 << l)) return false;
      if (l <= kLook) {
        for (int i = 0; i < cnt; ++i) {
          const int first = (code + i) << (kLook - l);
          for (int j = 0; j < (1 << (kLook - l)); ++j) t.look[first + j] = (uint16_t)((l << 8) | syms[k + i]);
        }
      }
      code += cnt;
      k += cnt;
      t.maxcode[l] = code - 1;
    } else {
      t.maxcode[l] = -1;
    }
    code <<= 1;
  }
  t.maxcode[17] = 0x7fffffff;
  t.defined = true;
  return true;
}

inline int be16(const uint8_t* p) { return (p[0] << 8) | p[1]; }

// Parses every marker segment up to and including SOS.  NST_OK, NST_E_SHAPE (not a fast-path stream) or NST_E_DATA.
int parse_header(const uint8_t* d, size_t len, Header& H, const char** why) {
#define FAIL(code, msg) \
  do {                  \
    *why = msg;         \
    return code;        \
  } while (0)
  if (len < 4 || d[0] != 0xFF || d[1] != 0xD8) FAIL(NST_E_SHAPE, "not a JPEG stream");
  size_t p = 2;
  bool have_sof = false;
  int comp_id[3] = {0, 0, 0}, comp_hv[3] = {0, 0, 0};
  for (;;) {
    if (p + 2 > len) FAIL(NST_E_DATA, "truncated before SOS");
    if (d[p] != 0xFF) FAIL(NST_E_DATA, "marker expected");
    while (p < len && d[p] == 0xFF) ++p;  // fill bytes
    if (p >= len) FAIL(NST_E_DATA, "truncated before SOS");
    const int m = d[p++];
    if (m == 0xD8 || m == 0xD9 || m == 0x00 || m == 0x01 || (m >= 0xD0 && m <= 0xD7))
      FAIL(NST_E_DATA, "unexpected marker before SOS");
    if (p + 2 > len) FAIL(NST_E_DATA, "truncated segment");
    const size_t L = (size_t)be16(d + p);
    if (L < 2 || p + L > len) FAIL(NST_E_DATA, "truncated segment");
    const uint8_t* s = d + p + 2;
    const size_t n = L - 2;
    if ((m >= 0xE0 && m <= 0xEF) || m == 0xFE) {
      if (m == 0xEE && n >= 5 && !memcmp(s, "Adobe", 5)) FAIL(NST_E_SHAPE, "Adobe APP14 stream");
    } else if (m == 0xDB) {
      size_t q = 0;
      while (q < n) {
        const int pq = s[q] >> 4, id = s[q] & 15;
        if (pq != 0) FAIL(NST_E_SHAPE, "16-bit quantisation table");
        if (id > 3 || q + 65 > n) FAIL(NST_E_DATA, "bad DQT");
        for (int i = 0; i < 64; ++i) H.qt[id][kZigzag[i]] = s[q + 1 + i];
        H.qt_defined[id] = true;
        q += 65;
      }
    } else if (m == 0xC4) {
      size_t q = 0;
      while (q < n) {
        if (q + 17 > n) FAIL(NST_E_DATA, "bad DHT");
        const int cls = s[q] >> 4, id = s[q] & 15;
        if (cls > 1 || id > 3) FAIL(NST_E_DATA, "bad DHT");
        int total = 0;
        for (int i = 0; i < 16; ++i) total += s[q + 1 + i];
        if (total > 256 || q + 17 + (size_t)total > n) FAIL(NST_E_DATA, "bad DHT");
        if (!build_table(cls ? H.ac[id] : H.dc[id], s + q + 1, s + q + 17, total)) FAIL(NST_E_DATA, "bad DHT codes");
        q += 17 + (size_t)total;
      }
    } else if (m == 0xC0) {
      if (have_sof) FAIL(NST_E_DATA, "two frame headers");
      if (n < 6) FAIL(NST_E_DATA, "bad SOF0");
      if (s[0] != 8) FAIL(NST_E_SHAPE, "sample precision is not 8");
      H.h = be16(s + 1);
      H.w = be16(s + 3);
      H.comps = s[5];
      if (H.h == 0) FAIL(NST_E_SHAPE, "height left to a DNL marker");
      if (H.w == 0) FAIL(NST_E_DATA, "zero width");
      if (H.comps != 1 && H.comps != 3) FAIL(NST_E_SHAPE, "neither 1 nor 3 components");
      if (n != 6 + 3 * (size_t)H.comps) FAIL(NST_E_DATA, "bad SOF0");
      for (int c = 0; c < H.comps; ++c) {
        comp_id[c] = s[6 + 3 * c];
        comp_hv[c] = s[7 + 3 * c];
        H.tq[c] = s[8 + 3 * c];
        const int ch = comp_hv[c] >> 4, cv = comp_hv[c] & 15;
        if (ch < 1 || ch > 4 || cv < 1 || cv > 4 || H.tq[c] > 3) FAIL(NST_E_DATA, "bad SOF0 component");
      }
      if (H.comps == 3) {
        if (comp_id[0] != 1 || comp_id[1] != 2 || comp_id[2] != 3) FAIL(NST_E_SHAPE, "component ids are not 1,2,3");
        if (comp_hv[1] != 0x11 || comp_hv[2] != 0x11) FAIL(NST_E_SHAPE, "chroma sampling is not 1x1");
        if (comp_hv[0] == 0x11) H.sampling = 0;
        else if (comp_hv[0] == 0x21) H.sampling = 1;
        else if (comp_hv[0] == 0x22) H.sampling = 2;
        else FAIL(NST_E_SHAPE, "luma sampling is not 1x1, 2x1 or 2x2");
      } else {
        H.sampling = 0;  // a single-component scan is not interleaved: its declared factors do not matter
      }
      have_sof = true;
    } else if (m == 0xDD) {
      if (n != 2) FAIL(NST_E_DATA, "bad DRI");
      H.restart = be16(s);
    } else if (m == 0xDA) {
      if (!have_sof) FAIL(NST_E_DATA, "SOS before SOF");
      if (n < 1) FAIL(NST_E_DATA, "bad SOS");
      const int ns = s[0];
      if (ns < 1 || ns > 4 || n != 4 + 2 * (size_t)ns) FAIL(NST_E_DATA, "bad SOS");
      if (ns != H.comps) FAIL(NST_E_SHAPE, "scan does not hold every component");
      for (int c = 0; c < ns; ++c) {
        if (s[1 + 2 * c] != comp_id[c]) FAIL(NST_E_SHAPE, "scan components out of frame order");
        H.td[c] = s[2 + 2 * c] >> 4;
        H.ta[c] = s[2 + 2 * c] & 15;
        if (H.td[c] > 3 || H.ta[c] > 3) FAIL(NST_E_DATA, "bad SOS table selector");
        if (!H.dc[H.td[c]].defined || !H.ac[H.ta[c]].defined) FAIL(NST_E_DATA, "scan names an undefined Huffman table");
        if (!H.qt_defined[H.tq[c]]) FAIL(NST_E_DATA, "component names an undefined quantisation table");
      }
      if (s[1 + 2 * ns] != 0 || s[2 + 2 * ns] != 63 || s[3 + 2 * ns] != 0) FAIL(NST_E_SHAPE, "not a sequential scan");
      H.scan_pos = p + L;
      if (!jpeg_geom(H.h, H.w, H.comps, H.sampling, &H.geom)) FAIL(NST_E_DATA, "bad geometry");
      return NST_OK;
    } else {
      // SOF1..15 (extended, progressive, lossless, arithmetic), DAC, DNL, DHP, EXP, JPGn, reserved
      FAIL(NST_E_SHAPE, "not a baseline Huffman stream");
    }
    p += L;
  }
#undef FAIL
}

// MSB-first bit reader over the entropy-coded segment.  At a marker or the end of the data it stops advancing and
// feeds zero bits, counting them: a clean stream never consumes one (checked at every restart and at the end).
struct BitReader {
  const uint8_t* d;
  size_t len, pos;
  uint64_t bits = 0;
  int n = 0;    // valid bits in the low end of `bits`
  int pad = 0;  // how many of them are made-up zeros (always the lowest)
  bool stopped = false;

  inline void refill() {
    if (n <= 32 && !stopped && pos + 4 <= len) {
      const uint32_t v = ((uint32_t)d[pos] << 24) | ((uint32_t)d[pos + 1] << 16) | ((uint32_t)d[pos + 2] << 8) | d[pos + 3];
      const uint32_t x = ~v;
      if (!((x - 0x01010101u) & ~x & 0x80808080u)) {  // no 0xFF among the four
        bits = (bits << 32) | v;
        n += 32;
        pos += 4;
        return;
      }
    }
    while (n <= 56) {
      uint8_t b = 0;
      if (!stopped) {
        if (pos >= len) {
          stopped = true;
        } else if (d[pos] != 0xFF) {
          b = d[pos++];
        } else if (pos + 1 < len && d[pos + 1] == 0x00) {
          b = 0xFF;
          pos += 2;
        } else {
          stopped = true;  // a marker (or a lone trailing 0xFF): pos stays on its 0xFF
        }
      }
      if (stopped) pad += 8;
      bits = (bits << 8) | b;
      n += 8;
    }
  }
  inline uint32_t peek(int nb) const { return (uint32_t)(bits >> (n - nb)) & ((1u << nb) - 1u); }
  inline void reset() {
    bits = 0;
    n = 0;
    pad = 0;
    stopped = false;
  }
};

// one Huffman symbol; -1 for a code no length matches.  Needs n >= 16.
inline int decode_symbol(BitReader& br, const HuffTable& t) {
  const uint16_t e = t.look[br.peek(kLook)];
  if (e) {
    br.n -= e >> 8;
    return e & 255;
  }
  for (int l = kLook + 1; l <= 16; ++l) {
    const int32_t code = (int32_t)br.peek(l);
    if (code <= t.maxcode[l]) {
      const int32_t idx = code + t.valoff[l];
      if (idx < 0 || idx > 255) return -1;
      br.n -= l;
      return t.vals[idx];
    }
  }
  return -1;
}

inline int extend(uint32_t v, int s) { return v < (1u << (s - 1)) ? (int)v - (1 << s) + 1 : (int)v; }

inline bool decode_block(BitReader& br, const HuffTable& dc, const HuffTable& ac, int& pred, int16_t* out) {
  memset(out, 0, 128);
  br.refill();
  int s = decode_symbol(br, dc);
  if (s < 0 || s > 11) return false;
  if (s) {
    const uint32_t v = br.peek(s);
    br.n -= s;
    pred += extend(v, s);
    if (pred < -32768 || pred > 32767) return false;
  }
  out[0] = (int16_t)pred;
  for (int k = 1; k < 64;) {
    br.refill();
    const int rs = decode_symbol(br, ac);
    if (rs < 0) return false;
    const int r = rs >> 4;
    s = rs & 15;
    if (!s) {
      if (r != 15) break;  // end of block
      k += 16;
      if (k > 64) return false;
      continue;
    }
    k += r;
    if (k > 63) return false;
    const uint32_t v = br.peek(s);
    br.n -= s;
    out[kZigzag[k]] = (int16_t)extend(v, s);
    ++k;
  }
  return true;
}

int decode_scan(const uint8_t* d, size_t len, const Header& H, uint8_t* record, const char** why) {
  const JpegGeom& g = H.geom;
  uint16_t* qt = (uint16_t*)record;
  memset(qt, 0, NST_JPEG_QT_BYTES);
  for (int c = 0; c < g.comps; ++c) memcpy(qt + 64 * c, H.qt[H.tq[c]], 128);
  int16_t* coef = (int16_t*)(record + NST_JPEG_QT_BYTES);
  BitReader br{d, len, H.scan_pos};
  const int mcux = g.comps == 1 ? g.bw[0] : g.bw[1], mcuy = g.comps == 1 ? g.bh[0] : g.bh[1];
  const size_t mcus = (size_t)mcux * mcuy;
  int pred[3] = {0, 0, 0};
  int togo = H.restart, rst = 0;
  size_t done = 0;
  for (int my = 0; my < mcuy; ++my) {
    for (int mx = 0; mx < mcux; ++mx) {
      for (int c = 0; c < g.comps; ++c) {
        const int nh = c == 0 ? g.hs : 1, nv = c == 0 ? g.vs : 1;
        for (int v = 0; v < nv; ++v)
          for (int hh = 0; hh < nh; ++hh) {
            const size_t b = g.blk_off[c] + (size_t)(my * nv + v) * g.bw[c] + (size_t)(mx * nh + hh);
            if (!decode_block(br, H.dc[H.td[c]], H.ac[H.ta[c]], pred[c], coef + b * 64)) {
              *why = "bad Huffman code or coefficient index";
              return NST_E_DATA;
            }
          }
      }
      ++done;
      if (H.restart && --togo == 0 && done < mcus) {
        // a restart marker follows: fewer than 8 (padding) bits may remain before it, none of them made up
        if (br.n - br.pad < 0 || br.n - br.pad > 7) {
          *why = "restart interval does not end at its marker";
          return NST_E_DATA;
        }
        size_t p = br.pos;
        if (p >= len || d[p] != 0xFF) {
          *why = "restart marker missing";
          return NST_E_DATA;
        }
        while (p < len && d[p] == 0xFF) ++p;
        if (p >= len || d[p] != 0xD0 + rst) {
          *why = "restart marker missing or out of sequence";
          return NST_E_DATA;
        }
        br.pos = p + 1;
        br.reset();
        rst = (rst + 1) & 7;
        togo = H.restart;
        pred[0] = pred[1] = pred[2] = 0;
      }
    }
  }
  if (br.n - br.pad < 0 || br.n - br.pad > 7) {
    *why = "scan does not end at EOI";
    return NST_E_DATA;
  }
  size_t p = br.pos;
  if (p >= len || d[p] != 0xFF) {
    *why = "EOI missing";
    return NST_E_DATA;
  }
  while (p < len && d[p] == 0xFF) ++p;
  if (p >= len || d[p] != 0xD9) {
    *why = "EOI missing";
    return NST_E_DATA;
  }
  return NST_OK;
}

}  // namespace

extern "C" int nst_jpeg_probe(const uint8_t* data, size_t len, int* h, int* w, int* comps, int* sampling,
                              size_t* record_bytes) {
  if (!data || !len || !h || !w || !comps || !sampling || !record_bytes) {
    set_error("nst_jpeg_probe: invalid arguments");
    return NST_E_INVALID;
  }
  Header H;
  const char* why = "";
  const int rc = parse_header(data, len, H, &why);
  if (rc != NST_OK) {
    set_error(std::string("nst_jpeg_probe: ") + why);
    return rc;
  }
  *h = H.h;
  *w = H.w;
  *comps = H.comps;
  *sampling = H.sampling;
  *record_bytes = jpeg_record_bytes(H.geom);
  return NST_OK;
}

extern "C" int nst_jpeg_entropy_decode(const uint8_t* data, size_t len, void* record, size_t record_bytes) {
  if (!data || !len || !record || !record_bytes || ((uintptr_t)record & 1)) {
    set_error("nst_jpeg_entropy_decode: invalid arguments (record 2-byte aligned)");
    return NST_E_INVALID;
  }
  Header H;
  const char* why = "";
  int rc = parse_header(data, len, H, &why);
  if (rc == NST_OK && record_bytes != jpeg_record_bytes(H.geom)) {
    set_error("nst_jpeg_entropy_decode: record_bytes is not what nst_jpeg_probe reports for this stream");
    return NST_E_INVALID;
  }
  if (rc == NST_OK) rc = decode_scan(data, len, H, (uint8_t*)record, &why);
  if (rc != NST_OK) set_error(std::string("nst_jpeg_entropy_decode: ") + why);
  return rc;
}
