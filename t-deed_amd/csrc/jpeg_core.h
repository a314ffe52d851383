// Baseline JPEG decode arithmetic shared by the device kernels (jpeg.hip) and the host check programs
// (tools/jpeg_host_check.cpp, tools/jpeg_split_check.cpp, tools/jpeg_stage_check.cpp): bit reader, Huffman symbol decode,
// the coefficient decode of a segment or of a piece of one (from a recorded decoder state), the integer "islow"
// IDCT, libjpeg's "fancy" triangle up-sampling taps and the integer YCbCr -> RGB conversion.  Everything is integer
// arithmetic and reproduces Pillow's Image.open(..).convert("RGB") (libjpeg-turbo) bit for bit on the supported subset
// (tdeed_amd/jpegdev.py: parse).  No HIP types here: the file also compiles with a plain host C++ compiler.
//
// Bounds: nothing in this file reads the entropy stream outside [off, off + len) of its segment, and nothing stores a
// coefficient outside the frame's own `frame_blocks * 64` int16 values; both hold for ANY stream bytes and ANY table
// contents (table indices are masked), which is what the host check program's sanitizer run exercises on damaged files.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define JC_HD static __host__ __device__ __forceinline__
#else
#define JC_HD static inline
#endif
#if defined(__HIPCC__)
#define JC_HD_MEMBER __host__ __device__ __forceinline__
#else
#define JC_HD_MEMBER inline
#endif
#if defined(__clang__)
#define JC_UNROLL _Pragma("unroll")
#else
#define JC_UNROLL
#endif

// chroma sampling of a frame (luma factors hs x vs; chroma is always 1 x 1)
enum { JC_GREY = 0, JC_444 = 1, JC_422 = 2, JC_420 = 3 };

// per-segment status
enum {
  JC_OK = 0,
  JC_ERR_EXHAUSTED = 1,   // data ran out before the last MCU of the segment
  JC_ERR_MARKER = 2,      // FF xx (xx != 00) inside the segment
  JC_ERR_CODE = 3,        // no Huffman code within 16 bits
  JC_ERR_DC = 4,          // DC category above 11
  JC_ERR_AC = 5,          // AC size above 10
  JC_ERR_RUN = 6,         // zero run takes k past 63
  JC_ERR_TABLE = 7        // a row of the segment table points outside its buffers
};

// One Huffman table in decode form: an 8-bit look-ahead (code length << 8 | symbol, 0 = longer than 8 bits) and the
// canonical slow path (largest code per length, -1 = none; vals[valoff[l] + code]).
struct JcHuff {
  uint16_t look[256];
  int32_t maxcode[18];
  int32_t valoff[18];
  uint8_t vals[256];
};

// Everything the tables of one encoder say: quantisers in natural order, Huffman tables DC0 DC1 AC0 AC1, the table
// selectors per component, and the zig-zag -> natural map (kept here so that the kernel finds it in LDS with the rest).
struct JcTableSet {
  uint16_t quant[4][64];
  JcHuff huff[4];
  uint8_t tq[4], td[4], ta[4];
  uint8_t natural[64];
  uint8_t pad[4];
};
#define JC_TABLE_SET_BYTES 4240
static_assert(sizeof(JcHuff) == 912, "JcHuff layout (jpegdev.py packs it with numpy)");
static_assert(sizeof(JcTableSet) == JC_TABLE_SET_BYTES && JC_TABLE_SET_BYTES % 16 == 0, "JcTableSet layout");

// One row of the segment table: a frame's scan, or one restart interval of it.
struct JcSegment {
  int32_t frame, first_mcu, n_mcu, offset, length, set;
};

// Block geometry of a frame: component c has bw[c] x bh[c] blocks (the padded MCU grid) stored row-major from block
// boff[c] of the frame's coefficient range; cw[c] x ch[c] is its down-sampled size, which the up-sampling edges follow.
struct JcGeom {
  int W, H, samp, ncomp, hs, vs, mcus_x, mcus_y, bpm, frame_blocks;
  int bw[3], bh[3], cw[3], ch[3], boff[3];
};

JC_HD JcGeom jc_geom(int W, int H, int samp) {
  JcGeom g;
  g.W = W; g.H = H; g.samp = samp;
  g.ncomp = samp == JC_GREY ? 1 : 3;
  g.hs = (samp == JC_422 || samp == JC_420) ? 2 : 1;
  g.vs = samp == JC_420 ? 2 : 1;
  g.mcus_x = (W + 8 * g.hs - 1) / (8 * g.hs);
  g.mcus_y = (H + 8 * g.vs - 1) / (8 * g.vs);
  g.bpm = g.ncomp == 1 ? 1 : g.hs * g.vs + 2;
  int off = 0;
  for (int c = 0; c < 3; ++c) {
    const int h = c == 0 ? g.hs : 1, v = c == 0 ? g.vs : 1;
    const bool live = c < g.ncomp;
    g.bw[c] = live ? g.mcus_x * h : 0;
    g.bh[c] = live ? g.mcus_y * v : 0;
    g.cw[c] = live ? (W * h + g.hs - 1) / g.hs : 0;
    g.ch[c] = live ? (H * v + g.vs - 1) / g.vs : 0;
    g.boff[c] = off;
    off += g.bw[c] * g.bh[c];
  }
  g.frame_blocks = off;
  return g;
}

// What a pixel pass over the window [top, top + wh) x [left, left + ww) of a frame reads (jpegdev.window_blocks states the
// same formulas): the bands (MCU rows) that hold window rows, the luma block columns and block rows under the window,
// the chroma block columns of the samples jc_pixel's taps touch -- for 2:1 chroma sample x >> 1 and its clamped
// neighbour, one to the left of an even x, one to the right of an odd x -- and the MCU rows whose coefficients are read:
// the bands, plus for 4:2:0 the band above when the window starts on a band's first row and the band below when it ends
// on a band's last row (the vertical taps' halo).  All ranges are inclusive lo / count or lo / hi.
struct JcWindow {
  int top, left, wh, ww;
  int band_lo, band_n;          // bands band_lo .. band_lo + band_n - 1
  int ybx_lo, ybx_n;            // luma block columns
  int ybr_lo, ybr_hi;           // luma block rows
  int cbx_lo, cbx_n;            // chroma block columns (0, 0 for greyscale)
  int mrow_lo, mrow_hi;         // MCU rows read, halo included
};

// the caller has checked 0 <= top, 0 < wh, top + wh <= H and the same for the columns
JC_HD JcWindow jc_window(const JcGeom& g, int top, int left, int wh, int ww) {
  JcWindow w;
  w.top = top; w.left = left; w.wh = wh; w.ww = ww;
  const int x1 = left + ww - 1, y1 = top + wh - 1;
  w.band_lo = top / (8 * g.vs);
  w.band_n = y1 / (8 * g.vs) - w.band_lo + 1;
  w.ybx_lo = left / 8;
  w.ybx_n = x1 / 8 - w.ybx_lo + 1;
  w.ybr_lo = top / 8;
  w.ybr_hi = y1 / 8;
  w.cbx_lo = w.cbx_n = 0;
  if (g.ncomp == 3) {
    int c_lo = left, c_hi = x1;
    if (g.hs == 2) {
      c_lo = (left & 1) ? left >> 1 : ((left >> 1) > 0 ? (left >> 1) - 1 : 0);
      c_hi = (x1 & 1) ? ((x1 >> 1) + 1 < g.cw[1] ? (x1 >> 1) + 1 : g.cw[1] - 1) : x1 >> 1;
    }
    w.cbx_lo = c_lo / 8;
    w.cbx_n = c_hi / 8 - w.cbx_lo + 1;
  }
  w.mrow_lo = w.band_lo;
  w.mrow_hi = w.band_lo + w.band_n - 1;
  if (g.vs == 2 && g.ncomp == 3) {
    if (top % 16 == 0 && w.mrow_lo > 0) --w.mrow_lo;
    if (y1 % 16 == 15 && (y1 >> 1) + 1 < g.ch[1]) ++w.mrow_hi;
  }
  return w;
}

// --------------------------------------------------------------------------------------------- bit reader
// Right-aligned 64-bit buffer with n valid bits.  Past the end of the segment (or behind a marker) it is fed zero
// bits, as libjpeg does; `pad` counts the zero bits at the tail, so n < pad after a symbol means it consumed some.
struct JcBits {
  uint64_t buf;
  int n, pad, marker;
  const uint8_t* p;
  const uint8_t* end;
};

// n >= 32 afterwards: enough for the longest symbol (16 code bits + 11 extra bits)
JC_HD void jc_refill(JcBits& b) {
  if (b.n >= 32) return;
  if (!b.marker && b.end - b.p >= 4) {
    uint32_t w;
    __builtin_memcpy(&w, b.p, 4);
    const uint32_t t = ~w;                                     // a zero byte of t is an FF byte of w
    if (((t - 0x01010101u) & ~t & 0x80808080u) == 0) {
      b.buf = (b.buf << 32) | __builtin_bswap32(w);
      b.n += 32;
      b.p += 4;
      return;
    }
  }
  for (int i = 0; i < 4; ++i) {
    uint32_t c = 0;
    bool real = false;
    if (!b.marker && b.p < b.end) {
      c = *b.p;
      if (c != 0xFF) {
        b.p += 1;
        real = true;
      } else if (b.end - b.p >= 2 && b.p[1] == 0) {            // stuffed FF 00
        b.p += 2;
        real = true;
      } else {                                                  // a marker, or a lone FF at the end: the data ends here
        b.marker = 1;
        c = 0;
      }
    }
    b.buf = (b.buf << 8) | c;
    b.n += 8;
    b.pad += real ? 0 : 8;
  }
}

JC_HD uint32_t jc_peek(const JcBits& b, int l) { return (uint32_t)(b.buf >> (b.n - l)) & ((1u << l) - 1u); }

// value of t extra bits v (t >= 1): the difference extension of the standard
JC_HD int jc_extend(uint32_t v, int t) { return (int)v < (1 << (t - 1)) ? (int)v - (1 << t) + 1 : (int)v; }

// one Huffman symbol; -1 when no code matches within 16 bits
JC_HD int jc_symbol(JcBits& b, const JcHuff* h) {
  const uint32_t e = h->look[jc_peek(b, 8)];
  int l = (int)(e >> 8);
  if (l > 0 && l <= 8) {
    b.n -= l;
    return (int)(e & 255u);
  }
  for (l = 9; l <= 16; ++l) {
    const int code = (int)jc_peek(b, l);
    if (code <= h->maxcode[l]) {
      b.n -= l;
      return h->vals[(h->valoff[l] + code) & 255];
    }
  }
  return -1;
}

// false when a row of the segment table cannot be decoded safely
JC_HD bool jc_segment_ok(const JcSegment& s, long stream_bytes, int n_sets, int total_mcus) {
  return s.offset >= 0 && s.length >= 0 && (long)s.offset + s.length <= stream_bytes && s.set >= 0 && s.set < n_sets &&
         s.first_mcu >= 0 && s.n_mcu > 0 && (long)s.first_mcu + s.n_mcu <= total_mcus;
}

// --------------------------------------------------------------------------------------------- decoder state, pieces
// What the bit reader and the MCU loop carry across an MCU boundary: the offset of the next unread byte inside the
// segment, the n valid bits of the buffer, pad and marker (jc_refill feeds zero bytes at the tail of a segment, so a
// boundary inside the last four bytes already has pad > 0, and one behind a marker has marker set) and the three DC
// predictors.  A decode that starts from a recorded state continues with the bits the whole-segment decode reads.
struct JcState {
  uint64_t bits;
  int32_t byte_off, n, pad, marker;
  int32_t pred[3];
  int32_t spare;
};

// One row of the piece table: the MCUs [first_mcu, first_mcu + n_mcu) of segment `segment`, decodable on their own.
// pos: position in the resident stream of the piece's next unread byte (the segment's start + st.byte_off); left: the
// bytes from there to the end of the segment.  jpegdev.py mirrors the layout (PIECE).
struct JcPiece {
  int64_t pos;
  int32_t segment, first_mcu, n_mcu, set, left, spare;
  JcState st;
};
#define JC_PIECE_BYTES 72
static_assert(sizeof(JcState) == 40 && sizeof(JcPiece) == JC_PIECE_BYTES && JC_PIECE_BYTES % 8 == 0,
              "JcPiece layout (jpegdev.py reads it with numpy)");

// false when a piece row cannot be decoded safely: byte range outside the stream, a foreign table set, MCUs outside the
// frame, or a bit buffer state no decode leaves behind (0 <= pad <= n <= 63)
JC_HD bool jc_piece_ok(const JcPiece& p, long stream_bytes, int n_sets, int total_mcus) {
  return p.pos >= 0 && p.left >= 0 && p.pos <= stream_bytes && (long)p.left <= stream_bytes - p.pos && p.set >= 0 &&
         p.set < n_sets && p.first_mcu >= 0 && p.n_mcu > 0 && (long)p.first_mcu + p.n_mcu <= total_mcus && p.st.n >= 0 &&
         p.st.n <= 63 && p.st.pad >= 0 && p.st.pad <= p.st.n && p.st.byte_off >= 0;
}

// One row of the relocation table of a coefficient slot (trainclips.stage_batch): the pieces decoded into the slot have
// their bytes at pos - delta of the device buffer -- a staged copy of a byte range of the set; delta = 0 where the stream
// is resident at its own position -- and may read the window [lo, hi) of that buffer only.
struct JcReloc {
  int64_t delta, lo, hi;
};
#define JC_RELOC_BYTES 24
static_assert(sizeof(JcReloc) == JC_RELOC_BYTES, "JcReloc layout (trainclips.py packs it with numpy)");

// false when the piece's bytes [pos - delta, pos - delta + left) do not lie wholly inside the slot's window, or the window
// not inside the buffer.  pos, lo and hi - left are not negative where they are subtracted, so nothing overflows whatever
// the row holds: pos - delta >= lo  <=>  delta <= pos - lo, and pos - delta + left <= hi  <=>  delta >= pos - (hi - left).
JC_HD bool jc_reloc_ok(const JcPiece& p, const JcReloc& r, long stream_bytes) {
  return p.pos >= 0 && p.left >= 0 && r.lo >= 0 && r.lo <= r.hi && r.hi <= (int64_t)stream_bytes && r.hi - r.lo >= p.left &&
         r.delta <= p.pos - r.lo && r.delta >= p.pos - (r.hi - p.left);
}

// jc_piece_ok of a relocated piece: the byte range is held against the slot's window (jc_reloc_ok), the rest as above
JC_HD bool jc_piece_reloc_ok(const JcPiece& p, const JcReloc& r, long stream_bytes, int n_sets, int total_mcus) {
  JcPiece q = p;
  q.pos = 0;                                                   // the absolute range check passes: left <= stream_bytes below
  return jc_reloc_ok(p, r, stream_bytes) && jc_piece_ok(q, stream_bytes, n_sets, total_mcus);
}

// the split rule (jpegdev.split_points): MCU m of a segment starts a new piece when first_mcu < m and m % split_mcus == 0
JC_HD int jc_piece_count(int first_mcu, int n_mcu, int split_mcus) {
  return 1 + (first_mcu + n_mcu - 1) / split_mcus - first_mcu / split_mcus;
}

// Recorders of jc_entropy_run: `on` decides at compile time whether split points are looked at all.
struct JcNoRecord {
  static constexpr bool on = false;
  JC_HD_MEMBER void operator()(int, const JcState&) const {}
};

// --------------------------------------------------------------------------------------------- MCUs of one segment
// Decodes n_mcu MCUs of one frame, from MCU first_mcu on and from the decoder state st0, out of data[0, len) -- the
// segment's bytes from st0's next unread byte on.  STORE: into `coef` (the frame's zero-filled coefficient range, natural
// order, un-dequantised); otherwise nothing is stored.  Rec::on: rec(m, state) is called at every MCU m the run passes
// with m % split_mcus == 0 (the state's byte_off counts from data).  One flat loop, one symbol per iteration: lanes of a
// wavefront that are in different blocks still meet at the top of every iteration.  The caller has checked the row
// (jc_segment_ok / jc_piece_ok).
template <bool STORE, class Rec>
JC_HD int jc_entropy_run(const uint8_t* data, int len, const JcState& st0, int first_mcu, int n_mcu, const JcTableSet* ts,
                         int samp, int mcus_x, int mcus_y, int16_t* coef, int split_mcus, Rec& rec) {
  const int hs = (samp == JC_422 || samp == JC_420) ? 2 : 1, vs = samp == JC_420 ? 2 : 1;
  const int nY = samp == JC_GREY ? 1 : hs * vs, bpm = samp == JC_GREY ? 1 : nY + 2;
  const int bw0 = mcus_x * hs;
  JcBits b;
  b.buf = st0.bits; b.n = st0.n; b.pad = st0.pad; b.marker = st0.marker; b.p = data; b.end = data + len;
  int my = first_mcu / mcus_x, mx = first_mcu - my * mcus_x;
  int mcu = 0, j = 0, k = 0, c = 0;
  int pred0 = st0.pred[0], pred1 = st0.pred[1], pred2 = st0.pred[2];
  int to_split = Rec::on ? split_mcus - first_mcu % split_mcus : 0;       // MCUs until the next split point
  long base = 0;
  for (;;) {
    jc_refill(b);
    if (k == 0) {
      c = j < nY ? 0 : j - nY + 1;
      if (c == 0) {
        const int v = hs == 2 ? j >> 1 : j, h = hs == 2 ? j & 1 : 0;
        base = ((long)(my * vs + v) * bw0 + mx * hs + h) * 64;
      } else {                                                  // chroma planes follow the luma plane
        base = ((long)bw0 * mcus_y * vs + (long)(c - 1) * mcus_x * mcus_y + (long)my * mcus_x + mx) * 64;
      }
    }
    const JcHuff* h = &ts->huff[(k == 0 ? ts->td[c & 3] : 2 + ts->ta[c & 3]) & 3];
    const int sym = jc_symbol(b, h);
    if (sym < 0) return JC_ERR_CODE;
    if (k == 0) {
      if (sym > 11) return JC_ERR_DC;
      int diff = 0;
      if (sym) {
        diff = jc_extend(jc_peek(b, sym), sym);
        b.n -= sym;
      }
      int pred = c == 0 ? pred0 : c == 1 ? pred1 : pred2;
      pred = (int)((uint32_t)pred + (uint32_t)diff);            // wraps on a damaged stream or row instead of overflowing
      pred0 = c == 0 ? pred : pred0;
      pred1 = c == 1 ? pred : pred1;
      pred2 = c == 2 ? pred : pred2;
      if (STORE) coef[base] = (int16_t)pred;
      k = 1;
    } else {
      const int r = sym >> 4, s = sym & 15;
      if (s) {
        k += r;
        if (k > 63) return JC_ERR_RUN;
        if (s > 10) return JC_ERR_AC;
        const int v = jc_extend(jc_peek(b, s), s);
        b.n -= s;
        if (STORE) coef[base + (ts->natural[k] & 63)] = (int16_t)v;
        k += 1;
      } else if (r == 15) {
        k += 16;
        if (k > 64) return JC_ERR_RUN;
      } else {
        k = 64;                                                 // end of block
      }
    }
    if (b.n < b.pad) return b.marker ? JC_ERR_MARKER : JC_ERR_EXHAUSTED;
    if (k >= 64) {
      k = 0;
      if (++j == bpm) {
        j = 0;
        if (++mcu == n_mcu) return JC_OK;
        if (++mx == mcus_x) {
          mx = 0;
          ++my;
        }
        if (Rec::on && --to_split == 0) {
          to_split = split_mcus;
          JcState st;
          st.bits = b.n ? b.buf & (~(uint64_t)0 >> (64 - b.n)) : 0;
          st.byte_off = (int32_t)(b.p - data); st.n = b.n; st.pad = b.pad; st.marker = b.marker;
          st.pred[0] = pred0; st.pred[1] = pred1; st.pred[2] = pred2;
          st.spare = 0;
          rec(first_mcu + mcu, st);
        }
      }
    }
  }
}

JC_HD JcState jc_zero_state() {
  JcState st;
  st.bits = 0; st.byte_off = 0; st.n = 0; st.pad = 0; st.marker = 0;
  st.pred[0] = st.pred[1] = st.pred[2] = 0;
  st.spare = 0;
  return st;
}

// One whole segment from its first byte: the zero-state, no-recording instance.
JC_HD int jc_entropy_segment(const uint8_t* seg, int len, int first_mcu, int n_mcu, const JcTableSet* ts, int samp, int mcus_x,
                             int mcus_y, int16_t* coef) {
  JcNoRecord rec;
  return jc_entropy_run<true>(seg, len, jc_zero_state(), first_mcu, n_mcu, ts, samp, mcus_x, mcus_y, coef, 1, rec);
}

// --------------------------------------------------------------------------------------------- IDCT
// libjpeg's jidctint ("islow"): 13-bit constants, the column pass keeps 2 extra bits.  The arithmetic runs in uint32 so
// that absurd coefficients of a damaged stream wrap instead of overflowing a signed int (same bits for real images).
JC_HD void jc_idct_1d(const uint32_t* i, uint32_t* o) {
  uint32_t z1 = (i[2] + i[6]) * 4433u;
  const uint32_t t2 = z1 - i[6] * 15137u, t3 = z1 + i[2] * 6270u;
  const uint32_t t0 = (i[0] + i[4]) << 13, t1 = (i[0] - i[4]) << 13;
  const uint32_t t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
  uint32_t a0 = i[7], a1 = i[5], a2 = i[3], a3 = i[1];
  z1 = a0 + a3;
  uint32_t z2 = a1 + a2, z3 = a0 + a2, z4 = a1 + a3;
  const uint32_t z5 = (z3 + z4) * 9633u;
  a0 *= 2446u; a1 *= 16819u; a2 *= 25172u; a3 *= 12299u;
  z1 *= (uint32_t)-7373; z2 *= (uint32_t)-20995;
  z3 = z3 * (uint32_t)-16069 + z5;
  z4 = z4 * (uint32_t)-3196 + z5;
  a0 += z1 + z3; a1 += z2 + z4; a2 += z2 + z3; a3 += z1 + z4;
  o[0] = t10 + a3; o[7] = t10 - a3;
  o[1] = t11 + a2; o[6] = t11 - a2;
  o[2] = t12 + a1; o[5] = t12 - a1;
  o[3] = t13 + a0; o[4] = t13 - a0;
}

JC_HD uint32_t jc_descale(uint32_t x, int s) { return (uint32_t)((int32_t)(x + (1u << (s - 1))) >> s); }
JC_HD int jc_clamp255(int v) { return v < 0 ? 0 : v > 255 ? 255 : v; }

// One block: coef (64 int16, natural order, 16-byte aligned) times quant, both passes, level shift and clamp.
// rows[2 r], rows[2 r + 1]: samples 0..3 and 4..7 of row r, first sample in the low byte.
JC_HD void jc_idct_block(const int16_t* coef, const uint16_t* quant, uint32_t* rows) {
  int16_t cc[64];
  uint32_t ws[64];
  const int16_t* src = (const int16_t*)__builtin_assume_aligned(coef, 16);
JC_UNROLL
  for (int r = 0; r < 8; ++r) __builtin_memcpy(cc + r * 8, src + r * 8, 16);
JC_UNROLL
  for (int col = 0; col < 8; ++col) {
    uint32_t in[8], out[8];
JC_UNROLL
    for (int r = 0; r < 8; ++r) in[r] = (uint32_t)(int32_t)cc[r * 8 + col] * (uint32_t)quant[r * 8 + col];
    jc_idct_1d(in, out);
JC_UNROLL
    for (int r = 0; r < 8; ++r) ws[r * 8 + col] = jc_descale(out[r], 11);
  }
JC_UNROLL
  for (int r = 0; r < 8; ++r) {
    uint32_t out[8];
    jc_idct_1d(ws + r * 8, out);
    uint32_t lo = 0, hi = 0;
JC_UNROLL
    for (int x = 0; x < 4; ++x) {
      lo |= (uint32_t)jc_clamp255((int32_t)jc_descale(out[x], 18) + 128) << (8 * x);
      hi |= (uint32_t)jc_clamp255((int32_t)jc_descale(out[x + 4], 18) + 128) << (8 * x);
    }
    rows[2 * r] = lo;
    rows[2 * r + 1] = hi;
  }
}

// --------------------------------------------------------------------------------------------- up-sampling and colour
JC_HD void jc_ycc_to_rgb(int y, int cb, int cr, int& r, int& g, int& b) {
  cb -= 128;
  cr -= 128;
  r = jc_clamp255(y + ((91881 * cr + 32768) >> 16));
  g = jc_clamp255(y + ((-22554 * cb - 46802 * cr + 32768) >> 16));
  b = jc_clamp255(y + ((116130 * cb + 32768) >> 16));
}

// RGB of pixel (x, y).  P.at(c, row, col) is sample (row, col) of component c's plane; cw x ch is the chroma planes'
// down-sampled size.  The triangle taps' neighbour is clamped to that size, which gives libjpeg's edge rules: the first
// and last column (and the rows above the first and below the last) see the edge sample itself.
template <int SAMP, class Planes>
JC_HD void jc_pixel(const Planes& P, int x, int y, int cw, int ch, int& r, int& g, int& b) {
  const int Y = P.at(0, y, x);
  if (SAMP == JC_GREY) {
    r = g = b = Y;
    return;
  }
  int cb, cr;
  if (SAMP == JC_444) {
    cb = P.at(1, y, x);
    cr = P.at(2, y, x);
  } else {
    const int i = x >> 1, odd = x & 1;
    const int nx = odd ? (i + 1 < cw ? i + 1 : cw - 1) : (i > 0 ? i - 1 : 0);
    if (SAMP == JC_422) {
      const int rnd = odd ? 2 : 1;
      cb = (3 * P.at(1, y, i) + P.at(1, y, nx) + rnd) >> 2;
      cr = (3 * P.at(2, y, i) + P.at(2, y, nx) + rnd) >> 2;
    } else {
      const int rr = y >> 1;
      const int ny = (y & 1) ? (rr + 1 < ch ? rr + 1 : ch - 1) : (rr > 0 ? rr - 1 : 0);
      const int rnd = odd ? 7 : 8;
      cb = (3 * (3 * P.at(1, rr, i) + P.at(1, ny, i)) + 3 * P.at(1, rr, nx) + P.at(1, ny, nx) + rnd) >> 4;
      cr = (3 * (3 * P.at(2, rr, i) + P.at(2, ny, i)) + 3 * P.at(2, rr, nx) + P.at(2, ny, nx) + rnd) >> 4;
    }
  }
  jc_ycc_to_rgb(Y, cb, cr, r, g, b);
}
