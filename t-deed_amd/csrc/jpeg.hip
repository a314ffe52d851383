// Baseline JPEG decode of a video's frames: entropy decode (one lane per segment) into an int16 coefficient buffer, then
// dequantisation, IDCT, up-sampling and colour conversion into the planar uint8 (n,3,H,W) layout of the resident-video
// consumers.  The arithmetic lives in jpeg_core.h (shared with tools/jpeg_host_check.cpp); tables and the packed stream
// come from tdeed_amd/jpegdev.py.  For entropy streams that stay on the device (trainclips.ResidentJpegClips) an index pass
// records decoder states inside the segments and the batches decode one lane per piece.
#include "common.h"
#include "jpeg_core.h"

// =========================================================================== entropy decode
// One wavefront per workgroup; waves[w] = (first row of the segment table, count <= 64).  The rows of a wavefront share
// one table set (jpegdev.PackedJpegs.waves), staged in LDS once.  Lane i decodes segment first + i: sequential inside
// the segment, one flat per-symbol loop (jc_entropy_segment), so lanes in different blocks re-converge every symbol.
// A lane reads only [offset, offset + length) of the stream and stores only inside its frame's coefficient range; a row
// that points outside the buffers, a frame outside [frame_lo, frame_lo + n_frames) or a foreign table set gets
// JC_ERR_TABLE and touches nothing.  status[row] = 0 or the JC_ERR_* code.
__global__ __launch_bounds__(64) void jpeg_entropy_kernel(const uint8_t* __restrict__ stream, long stream_bytes,
                                                          const JcSegment* __restrict__ segs, int n_segments,
                                                          const int* __restrict__ waves, const JcTableSet* __restrict__ sets,
                                                          int n_sets, int samp, int mcus_x, int mcus_y, int frame_lo, int n_frames,
                                                          long frame_coefs, int16_t* __restrict__ coef, int* __restrict__ status) {
  __shared__ __attribute__((aligned(16))) JcTableSet ts;
  const int lane = threadIdx.x;
  int first = waves[2 * blockIdx.x], count = waves[2 * blockIdx.x + 1];
  if (first < 0 || first >= n_segments) return;
  count = count < 64 ? count : 64;
  count = count < n_segments - first ? count : n_segments - first;
  const int set = segs[first].set;
  if (set < 0 || set >= n_sets) {
    if (lane < count) status[first + lane] = JC_ERR_TABLE;
    return;
  }
  const u32x4* src = reinterpret_cast<const u32x4*>(sets + set);
  u32x4* dst = reinterpret_cast<u32x4*>(&ts);
  for (int i = lane; i < JC_TABLE_SET_BYTES / 16; i += 64) dst[i] = src[i];
  __syncthreads();
  if (lane >= count) return;
  const JcSegment s = segs[first + lane];
  const long f = (long)s.frame - frame_lo;
  if (!jc_segment_ok(s, stream_bytes, n_sets, mcus_x * mcus_y) || s.set != set || f < 0 || f >= n_frames) {
    status[first + lane] = JC_ERR_TABLE;
    return;
  }
  status[first + lane] =
      jc_entropy_segment(stream + s.offset, s.length, s.first_mcu, s.n_mcu, &ts, samp, mcus_x, mcus_y, coef + f * frame_coefs);
}

extern "C" int tdeed_jpeg_entropy(const uint8_t* stream, long stream_bytes, const int* segments, int n_segments, const int* waves,
                                  int n_waves, const uint8_t* table_sets, int n_sets, int W, int H, int sampling, int frame_lo,
                                  int n_frames, int16_t* coeff, int* status, void* hip_stream) {
  TD_CHECK(stream && segments && waves && table_sets && coeff && status, "jpeg_entropy: null pointer");
  TD_CHECK(stream_bytes > 0 && n_segments > 0 && n_waves > 0 && n_sets > 0 && n_frames > 0 && frame_lo >= 0,
           "jpeg_entropy: bad sizes");
  TD_CHECK(W > 0 && H > 0 && W <= 65535 && H <= 65535, "jpeg_entropy: bad frame size %dx%d", H, W);
  TD_CHECK(sampling >= JC_GREY && sampling <= JC_420, "jpeg_entropy: sampling %d (0 grey, 1 4:4:4, 2 4:2:2, 3 4:2:0)", sampling);
  TD_CHECK((((uintptr_t)table_sets) & 15) == 0 && (((uintptr_t)segments | (uintptr_t)waves | (uintptr_t)status) & 3) == 0 &&
               (((uintptr_t)coeff) & 15) == 0,
           "jpeg_entropy: table sets and coefficients must be 16-byte aligned, the tables 4-byte");
  const JcGeom g = jc_geom(W, H, sampling);
  hipLaunchKernelGGL(jpeg_entropy_kernel, dim3(n_waves), dim3(64), 0, (hipStream_t)hip_stream, stream, stream_bytes,
                     (const JcSegment*)segments, n_segments, waves, (const JcTableSet*)table_sets, n_sets, sampling, g.mcus_x,
                     g.mcus_y, frame_lo, n_frames, (long)g.frame_blocks * 64, coeff, status);
  TD_LAUNCH_CHECK("jpeg_entropy");
  return TDEED_OK;
}

// =========================================================================== resident streams: index pass and pieces
// The streams of a training set stay on the device (trainclips.ResidentJpegClips) and every batch decodes the frames it
// drew.  A frame without restart markers is one segment, one lane; so one pass at construction walks every segment
// (one lane per segment, as above, nothing stored) and records the decoder state at the split points of the segment
// (jc_piece_count's rule): the rows of the piece table, which the batches then decode one lane per piece.
// Row k of segment row i lands in pieces[piece_off[i] + k], as long as that stays below piece_off[i + 1] and n_pieces.
struct PieceWriter {
  static constexpr bool on = true;
  JcPiece* rows;
  long seg_pos;
  int room, k, seg_len, segment, set, end_mcu, split;
  __device__ __forceinline__ void operator()(int m, const JcState& st) {
    if (k < room) {
      JcPiece p;
      p.pos = seg_pos + st.byte_off;
      p.segment = segment; p.first_mcu = m; p.set = set; p.spare = 0;
      const int to_next = split - m % split;
      p.n_mcu = to_next < end_mcu - m ? to_next : end_mcu - m;
      p.left = seg_len - st.byte_off;
      p.st = st;
      rows[k] = p;
    }
    ++k;
  }
};

// segs / waves / piece_off / status: the rows of one shard (jpegdev.pack_frames), whose offsets count from stream + base;
// seg_base: the shard's first row in the set's segment numbering (what the piece rows carry)
__global__ __launch_bounds__(64) void jpeg_entropy_index_kernel(const uint8_t* __restrict__ stream, long stream_bytes, long base,
                                                                const JcSegment* __restrict__ segs, int n_segments,
                                                                const int* __restrict__ waves, const JcTableSet* __restrict__ sets,
                                                                int n_sets, int samp, int mcus_x, int mcus_y, int split_mcus,
                                                                const int* __restrict__ piece_off, int seg_base,
                                                                JcPiece* __restrict__ pieces, int n_pieces, int* __restrict__ status) {
  __shared__ __attribute__((aligned(16))) JcTableSet ts;
  const int lane = threadIdx.x;
  int first = waves[2 * blockIdx.x], count = waves[2 * blockIdx.x + 1];
  if (first < 0 || first >= n_segments) return;
  count = count < 64 ? count : 64;
  count = count < n_segments - first ? count : n_segments - first;
  const int set = segs[first].set;
  if (set < 0 || set >= n_sets) {
    if (lane < count) status[first + lane] = JC_ERR_TABLE;
    return;
  }
  const u32x4* src = reinterpret_cast<const u32x4*>(sets + set);
  u32x4* dst = reinterpret_cast<u32x4*>(&ts);
  for (int i = lane; i < JC_TABLE_SET_BYTES / 16; i += 64) dst[i] = src[i];
  __syncthreads();
  if (lane >= count) return;
  const int row = first + lane;
  const JcSegment s = segs[row];
  const int p_lo = piece_off[row], p_hi = piece_off[row + 1];
  if (!jc_segment_ok(s, stream_bytes - base, n_sets, mcus_x * mcus_y) || s.set != set || p_lo < 0 || p_hi <= p_lo ||
      p_hi > n_pieces) {
    status[row] = JC_ERR_TABLE;
    return;
  }
  PieceWriter w;
  w.rows = pieces + p_lo; w.room = p_hi - p_lo; w.k = 0;
  w.seg_pos = base + s.offset; w.seg_len = s.length; w.segment = seg_base + row; w.set = set;
  w.end_mcu = s.first_mcu + s.n_mcu; w.split = split_mcus;
  const JcState zero = jc_zero_state();
  {                                                            // the first piece starts where the segment does
    JcPiece p;
    p.pos = w.seg_pos;
    p.segment = w.segment; p.first_mcu = s.first_mcu; p.set = set; p.spare = 0;
    const int to_next = split_mcus - s.first_mcu % split_mcus;
    p.n_mcu = to_next < s.n_mcu ? to_next : s.n_mcu;
    p.left = s.length;
    p.st = zero;
    w.rows[0] = p;
    w.k = 1;
  }
  status[row] = jc_entropy_run<false>(stream + base + s.offset, s.length, zero, s.first_mcu, s.n_mcu, &ts, samp, mcus_x, mcus_y,
                                      (int16_t*)nullptr, split_mcus, w);
}

// items[i] = (piece row, coefficient slot); waves[w] = (first item, count <= 64), the items of a wavefront sharing one
// table set (trainclips.batch_tables).  Lane i decodes its piece into slot s's coefficient range, s in [slot_lo, slot_lo +
// n_slots).  An item or a piece row that points outside any buffer, or whose set is not the wavefront's, counts as
// JC_ERR_TABLE and touches nothing.  No status leaves the device per item: bit `code` of *err is set for every code met.
// RELOC (tdeed_jpeg_entropy_items_reloc): the same body, but a piece's bytes are a staged copy: reloc[s], s the item's
// slot, s < n_reloc, says how far below JcPiece.pos they lie in `stream` and which window of it the slot may read
// (jc_piece_reloc_ok); a piece that leaves its window, or a slot without a row, counts as JC_ERR_TABLE like the others.
template <bool RELOC>
__global__ __launch_bounds__(64) void jpeg_entropy_items_kernel(const uint8_t* __restrict__ stream, long stream_bytes,
                                                                const JcPiece* __restrict__ pieces, int n_pieces,
                                                                const int* __restrict__ items, int n_items,
                                                                const int* __restrict__ waves, const JcTableSet* __restrict__ sets,
                                                                int n_sets, int samp, int mcus_x, int mcus_y, int slot_lo, int n_slots,
                                                                long frame_coefs, int16_t* __restrict__ coef,
                                                                unsigned* __restrict__ err, const JcReloc* __restrict__ reloc,
                                                                int n_reloc) {
  __shared__ __attribute__((aligned(16))) JcTableSet ts;
  const int lane = threadIdx.x;
  int first = waves[2 * blockIdx.x], count = waves[2 * blockIdx.x + 1];
  if (first < 0 || first >= n_items || count <= 0) {
    if (lane == 0) atomicOr(err, 1u << JC_ERR_TABLE);
    return;
  }
  count = count < 64 ? count : 64;
  count = count < n_items - first ? count : n_items - first;
  const int p0 = items[2 * first];
  const int set = p0 >= 0 && p0 < n_pieces ? pieces[p0].set : -1;
  if (set < 0 || set >= n_sets) {
    if (lane == 0) atomicOr(err, 1u << JC_ERR_TABLE);
    return;
  }
  const u32x4* src = reinterpret_cast<const u32x4*>(sets + set);
  u32x4* dst = reinterpret_cast<u32x4*>(&ts);
  for (int i = lane; i < JC_TABLE_SET_BYTES / 16; i += 64) dst[i] = src[i];
  __syncthreads();
  if (lane >= count) return;
  const int pi = items[2 * (first + lane)];
  const int slot = items[2 * (first + lane) + 1];
  const long f = (long)slot - slot_lo;
  int st = JC_ERR_TABLE;
  if (pi >= 0 && pi < n_pieces && f >= 0 && f < n_slots && (!RELOC || slot < n_reloc)) {
    const JcPiece p = pieces[pi];
    long at = p.pos;
    bool ok;
    if (RELOC) {
      const JcReloc r = reloc[slot];
      ok = jc_piece_reloc_ok(p, r, stream_bytes, n_sets, mcus_x * mcus_y);
      at = p.pos - r.delta;
    } else {
      ok = jc_piece_ok(p, stream_bytes, n_sets, mcus_x * mcus_y);
    }
    if (ok && p.set == set) {
      JcNoRecord rec;
      st = jc_entropy_run<true>(stream + at, p.left, p.st, p.first_mcu, p.n_mcu, &ts, samp, mcus_x, mcus_y,
                                coef + f * frame_coefs, 1, rec);
    }
  }
  if (st != JC_OK) atomicOr(err, 1u << st);
}

static int jpeg_resident_checks(const char* who, const void* stream, long stream_bytes, const void* waves, int n_waves,
                                const void* table_sets, int n_sets, int W, int H, int sampling) {
  TD_CHECK(stream && waves && table_sets, "%s: null pointer", who);
  TD_CHECK(stream_bytes > 0 && n_waves > 0 && n_sets > 0, "%s: bad sizes", who);
  TD_CHECK(W > 0 && H > 0 && W <= 65535 && H <= 65535, "%s: bad frame size %dx%d", who, H, W);
  TD_CHECK(sampling >= JC_GREY && sampling <= JC_420, "%s: sampling %d (0 grey, 1 4:4:4, 2 4:2:2, 3 4:2:0)", who, sampling);
  TD_CHECK((((uintptr_t)table_sets) & 15) == 0 && (((uintptr_t)waves) & 3) == 0,
           "%s: table sets must be 16-byte aligned, the tables 4-byte", who);
  return TDEED_OK;
}

extern "C" int tdeed_jpeg_entropy_index(const uint8_t* stream, long stream_bytes, long base, const int* segments, int n_segments,
                                        const int* waves, int n_waves, const uint8_t* table_sets, int n_sets, int W, int H,
                                        int sampling, int split_mcus, const int* piece_off, int seg_base, void* pieces,
                                        int n_pieces, int* status, void* hip_stream) {
  const int rc = jpeg_resident_checks("jpeg_entropy_index", stream, stream_bytes, waves, n_waves, table_sets, n_sets, W, H, sampling);
  if (rc != TDEED_OK) return rc;
  TD_CHECK(segments && piece_off && pieces && status, "jpeg_entropy_index: null pointer");
  TD_CHECK(n_segments > 0 && n_pieces > 0 && seg_base >= 0 && base >= 0 && base <= stream_bytes, "jpeg_entropy_index: bad sizes");
  TD_CHECK(split_mcus > 0, "jpeg_entropy_index: split_mcus %d", split_mcus);
  TD_CHECK((((uintptr_t)segments | (uintptr_t)piece_off | (uintptr_t)status) & 3) == 0 && (((uintptr_t)pieces) & 7) == 0,
           "jpeg_entropy_index: the tables must be 4-byte aligned, the piece table 8-byte");
  const JcGeom g = jc_geom(W, H, sampling);
  hipLaunchKernelGGL(jpeg_entropy_index_kernel, dim3(n_waves), dim3(64), 0, (hipStream_t)hip_stream, stream, stream_bytes, base,
                     (const JcSegment*)segments, n_segments, waves, (const JcTableSet*)table_sets, n_sets, sampling, g.mcus_x,
                     g.mcus_y, split_mcus, piece_off, seg_base, (JcPiece*)pieces, n_pieces, status);
  TD_LAUNCH_CHECK("jpeg_entropy_index");
  return TDEED_OK;
}

extern "C" int tdeed_jpeg_entropy_items(const uint8_t* stream, long stream_bytes, const void* pieces, int n_pieces,
                                        const int* items, int n_items, const int* waves, int n_waves, const uint8_t* table_sets,
                                        int n_sets, int W, int H, int sampling, int slot_lo, int n_slots, int16_t* coeff,
                                        unsigned* err, void* hip_stream) {
  const int rc = jpeg_resident_checks("jpeg_entropy_items", stream, stream_bytes, waves, n_waves, table_sets, n_sets, W, H, sampling);
  if (rc != TDEED_OK) return rc;
  TD_CHECK(pieces && items && coeff && err, "jpeg_entropy_items: null pointer");
  TD_CHECK(n_pieces > 0 && n_items > 0 && slot_lo >= 0 && n_slots > 0, "jpeg_entropy_items: bad sizes");
  TD_CHECK((((uintptr_t)items | (uintptr_t)err) & 3) == 0 && (((uintptr_t)pieces) & 7) == 0 && (((uintptr_t)coeff) & 15) == 0,
           "jpeg_entropy_items: coefficients must be 16-byte aligned, the piece table 8-byte, the tables 4-byte");
  const JcGeom g = jc_geom(W, H, sampling);
  hipLaunchKernelGGL(jpeg_entropy_items_kernel<false>, dim3(n_waves), dim3(64), 0, (hipStream_t)hip_stream, stream, stream_bytes,
                     (const JcPiece*)pieces, n_pieces, items, n_items, waves, (const JcTableSet*)table_sets, n_sets, sampling,
                     g.mcus_x, g.mcus_y, slot_lo, n_slots, (long)g.frame_blocks * 64, coeff, err, (const JcReloc*)nullptr, 0);
  TD_LAUNCH_CHECK("jpeg_entropy_items");
  return TDEED_OK;
}

// tdeed_jpeg_entropy_items over staged copies: reloc holds n_reloc rows of (int64 delta, lo, hi), indexed by the item's slot
extern "C" int tdeed_jpeg_entropy_items_reloc(const uint8_t* stream, long stream_bytes, const void* pieces, int n_pieces,
                                              const int* items, int n_items, const int* waves, int n_waves,
                                              const uint8_t* table_sets, int n_sets, int W, int H, int sampling, int slot_lo,
                                              int n_slots, const void* reloc, int n_reloc, int16_t* coeff, unsigned* err,
                                              void* hip_stream) {
  const int rc =
      jpeg_resident_checks("jpeg_entropy_items_reloc", stream, stream_bytes, waves, n_waves, table_sets, n_sets, W, H, sampling);
  if (rc != TDEED_OK) return rc;
  TD_CHECK(pieces && items && coeff && err && reloc, "jpeg_entropy_items_reloc: null pointer");
  TD_CHECK(n_pieces > 0 && n_items > 0 && slot_lo >= 0 && n_slots > 0 && n_reloc > 0, "jpeg_entropy_items_reloc: bad sizes");
  TD_CHECK((((uintptr_t)items | (uintptr_t)err) & 3) == 0 && (((uintptr_t)pieces | (uintptr_t)reloc) & 7) == 0 &&
               (((uintptr_t)coeff) & 15) == 0,
           "jpeg_entropy_items_reloc: coefficients must be 16-byte aligned, the piece and relocation tables 8-byte, the tables "
           "4-byte");
  const JcGeom g = jc_geom(W, H, sampling);
  hipLaunchKernelGGL(jpeg_entropy_items_kernel<true>, dim3(n_waves), dim3(64), 0, (hipStream_t)hip_stream, stream, stream_bytes,
                     (const JcPiece*)pieces, n_pieces, items, n_items, waves, (const JcTableSet*)table_sets, n_sets, sampling,
                     g.mcus_x, g.mcus_y, slot_lo, n_slots, (long)g.frame_blocks * 64, coeff, err, (const JcReloc*)reloc, n_reloc);
  TD_LAUNCH_CHECK("jpeg_entropy_items_reloc");
  return TDEED_OK;
}

// Rows of a batch slot that no decode fills: fill[row] = -2 leaves the row alone, -1 zeroes it (a clip's padding), r >= 0
// copies row r of the side buffer (frames kept decoded: another sampling, outside the decoder's subset, damaged).
// blockIdx.y = row; a side row outside [0, side_rows) stores nothing.
template <class V>
__global__ __launch_bounds__(256) void jpeg_slot_fill_kernel(const V* __restrict__ side, long side_rows, long units,
                                                             const int* __restrict__ fill, V* __restrict__ out) {
  const int row = blockIdx.y;
  const int r = fill[row];
  if (r < -1 || r >= side_rows) return;
  const V* src = side + (long)(r < 0 ? 0 : r) * units;
  V* dst = out + (long)row * units;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < units; i += (long)gridDim.x * 256) dst[i] = r < 0 ? V{} : src[i];
}

extern "C" int tdeed_jpeg_slot_fill(const uint8_t* side, long side_rows, long frame_bytes, const int* fill, int n_rows,
                                    uint8_t* out, void* hip_stream) {
  TD_CHECK(fill && out && (side || side_rows == 0), "jpeg_slot_fill: null pointer");
  TD_CHECK(side_rows >= 0 && frame_bytes > 0 && n_rows > 0 && n_rows <= 65535, "jpeg_slot_fill: bad sizes");
  TD_CHECK((((uintptr_t)fill) & 3) == 0, "jpeg_slot_fill: fill must be 4-byte aligned");
  hipStream_t st = (hipStream_t)hip_stream;
  const bool v16 = frame_bytes % 16 == 0 && (((uintptr_t)side | (uintptr_t)out) & 15) == 0;
  const long units = v16 ? frame_bytes / 16 : frame_bytes;
  const long gx = cdiv(units, 256 * 4);
  const dim3 grid((unsigned)(gx < 64 ? gx : 64), n_rows);
  if (v16)
    hipLaunchKernelGGL(jpeg_slot_fill_kernel<u32x4>, grid, dim3(256), 0, st, (const u32x4*)side, side_rows, units, fill, (u32x4*)out);
  else
    hipLaunchKernelGGL(jpeg_slot_fill_kernel<uint8_t>, grid, dim3(256), 0, st, side, side_rows, units, fill, out);
  TD_LAUNCH_CHECK("jpeg_slot_fill");
  return TDEED_OK;
}

extern "C" long tdeed_jpeg_frame_coeffs(int W, int H, int sampling) {
  if (W <= 0 || H <= 0 || W > 65535 || H > 65535 || sampling < JC_GREY || sampling > JC_420) return -1;
  return (long)jc_geom(W, H, sampling).frame_blocks * 64;
}

// =========================================================================== pixels
// Workgroup (band, frame): one MCU row of the frame.  Phase 1: one thread per block runs dequantisation and both IDCT
// passes and writes the samples into LDS planes -- luma 8 VS rows, chroma 8 rows, and for 4:2:0 one chroma row above and
// below the band (the up-sampling taps reach one chroma sample across the MCU border), taken from a recomputed IDCT of
// the neighbouring band's chroma blocks.  Phase 2: one thread per 16 pixels of a row: triangle taps, colour conversion,
// three 16-byte stores (V16) or guarded byte stores.
// The frame lands in row dst_row[frame] of out when ROWS (tdeed_jpeg_pixels_rows: the frames of a clip batch go to rows
// i * T + t of the batch slot), in row frame otherwise; a row outside [0, out_rows) stores nothing.
// WIN (tdeed_jpeg_pixels_window): the same body over the window `win` of the frame (jc_window).  The grid holds the
// window's bands only, phase 1 runs the blocks jc_window lists and no others -- the LDS planes are as wide as those block
// columns, BandPlanes carries their first column -- and phase 2 covers the window's pixels, written as rows of a
// (wh, ww) plane.  Without WIN the window is the frame, the block columns are the padded MCU grid's (bw0, mcus_x) and every
// range below is the constant it was; jpeg_pixels_lds_bytes sizes the planes from the same columns.
struct BandPlanes {
  const uint8_t* y;
  const uint8_t* cb;
  const uint8_t* cr;
  int ypitch, cpitch, y0, c0;      // luma row y0 / chroma row c0 is row 0 of the LDS plane
  int yx0, cx0;                    // luma / chroma column that is column 0 of the LDS plane
  __device__ __forceinline__ int at(int c, int row, int col) const {
    return c == 0 ? y[(row - y0) * ypitch + col - yx0] : (c == 1 ? cb : cr)[(row - c0) * cpitch + col - cx0];
  }
};

template <int SAMP, bool V16, bool ROWS, bool WIN>
__global__ __launch_bounds__(256) void jpeg_pixels_kernel(const int16_t* __restrict__ coef, const int* __restrict__ frame_set,
                                                          const JcTableSet* __restrict__ sets, int n_sets, int frame_lo,
                                                          int W, int H, int mcus_x, int mcus_y, uint8_t* __restrict__ out,
                                                          const int* __restrict__ dst_row, long out_rows, const JcWindow win) {
  extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
  constexpr int HS = (SAMP == JC_422 || SAMP == JC_420) ? 2 : 1, VS = SAMP == JC_420 ? 2 : 1;
  constexpr int NC = SAMP == JC_GREY ? 0 : 2;                 // chroma planes
  constexpr int HALO = SAMP == JC_420 ? 1 : 0;
  constexpr int CROWS = 8 + 2 * HALO;
  const int band = (WIN ? win.band_lo : 0) + blockIdx.x, fl = blockIdx.y;
  const int set = frame_set[frame_lo + fl];
  if (set < 0 || set >= n_sets) return;                        // a frame that is decoded on the host
  const long row = ROWS ? (long)dst_row[frame_lo + fl] : (long)frame_lo + fl;
  if (ROWS && (row < 0 || row >= out_rows)) return;            // a frame that no row of the slot takes
  TD_DEV_ASSERT(row >= 0 && (!ROWS || row < out_rows));
  const JcTableSet* ts = sets + set;
  const int bw0 = mcus_x * HS;
  const int ybx_lo = WIN ? win.ybx_lo : 0, ybx_n = WIN ? win.ybx_n : bw0;       // the block columns phase 1 runs
  const int cbx_lo = WIN ? win.cbx_lo : 0, cbx_n = WIN ? win.cbx_n : mcus_x;
  const int ypitch = ybx_n * 8, cpitch = cbx_n * 8;
  uint8_t* ly = lds;
  uint8_t* lc = lds + 8 * VS * ypitch;                         // [NC][CROWS][cpitch]
  const long luma_blocks = (long)bw0 * mcus_y * VS, chroma_blocks = (long)mcus_x * mcus_y;
  const int16_t* fc = coef + (long)fl * (luma_blocks + NC * chroma_blocks) * 64;

  const int nY = VS * ybx_n, crows_b = 1 + 2 * HALO, nC = NC * crows_b * cbx_n;
  for (int t = threadIdx.x; t < nY + nC; t += 256) {
    uint32_t rows[16];
    if (t < nY) {
      const int v = t / ybx_n, bx = t - v * ybx_n;
      if (WIN && (band * VS + v < win.ybr_lo || band * VS + v > win.ybr_hi)) continue;   // a block row outside the window
      jc_idct_block(fc + ((long)(band * VS + v) * bw0 + ybx_lo + bx) * 64, ts->quant[ts->tq[0] & 3], rows);
#pragma unroll
      for (int r = 0; r < 8; ++r)
        *reinterpret_cast<u32x2*>(ly + (v * 8 + r) * ypitch + bx * 8) = (u32x2){rows[2 * r], rows[2 * r + 1]};
    } else {
      const int u = t - nY, per = crows_b * cbx_n;
      const int c = u / per, w = u - c * per, rel = w / cbx_n, bx = w - rel * cbx_n;
      const int by = band + rel - HALO;                        // rel 0 / 2 of 4:2:0: the band above / below
      if (by < 0 || by >= mcus_y) continue;
      if (WIN && (by < win.mrow_lo || by > win.mrow_hi)) continue;                       // a halo row no window pixel taps
      jc_idct_block(fc + (luma_blocks + c * chroma_blocks + (long)by * mcus_x + cbx_lo + bx) * 64, ts->quant[ts->tq[1 + c] & 3],
                    rows);
      uint8_t* plane = lc + c * CROWS * cpitch + bx * 8;
      if (HALO && rel == 0) {
        *reinterpret_cast<u32x2*>(plane) = (u32x2){rows[14], rows[15]};
      } else if (HALO && rel == 2) {
        *reinterpret_cast<u32x2*>(plane + 9 * cpitch) = (u32x2){rows[0], rows[1]};
      } else {
#pragma unroll
        for (int r = 0; r < 8; ++r)
          *reinterpret_cast<u32x2*>(plane + (HALO + r) * cpitch) = (u32x2){rows[2 * r], rows[2 * r + 1]};
      }
    }
  }
  __syncthreads();

  BandPlanes P;
  P.y = ly; P.cb = lc; P.cr = lc + CROWS * cpitch;
  P.ypitch = ypitch; P.cpitch = cpitch;
  P.y0 = band * 8 * VS; P.c0 = band * 8 - HALO;
  P.yx0 = ybx_lo * 8; P.cx0 = cbx_lo * 8;
  const int cw = (W + HS - 1) / HS, ch = (H + VS - 1) / VS;
  const int top = WIN ? win.top : 0, left = WIN ? win.left : 0, wh = WIN ? win.wh : H, ww = WIN ? win.ww : W;
  const int y_lo = band * 8 * VS > top ? band * 8 * VS : top;                            // the band's rows inside the window
  const int y_end = (band + 1) * 8 * VS < top + wh ? (band + 1) * 8 * VS : top + wh;
  const int rows_here = y_end - y_lo;
  const int chunks = (ww + 15) / 16;
  const long plane_px = (long)wh * ww;
  uint8_t* of = out + row * 3 * plane_px;
  for (int t = threadIdx.x; t < rows_here * chunks; t += 256) {
    const int ry = t / chunks, x0 = (t - ry * chunks) * 16, y = y_lo + ry;
    uint32_t pr[4] = {0, 0, 0, 0}, pg[4] = {0, 0, 0, 0}, pb[4] = {0, 0, 0, 0};
    uint8_t* o = of + (long)(y - top) * ww + x0;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      if (V16 || x0 + i < ww) {
        int r, g, b;
        jc_pixel<SAMP>(P, left + x0 + i, y, cw, ch, r, g, b);
        if (V16) {
          pr[i >> 2] |= (uint32_t)r << (8 * (i & 3));
          pg[i >> 2] |= (uint32_t)g << (8 * (i & 3));
          pb[i >> 2] |= (uint32_t)b << (8 * (i & 3));
        } else {
          o[i] = (uint8_t)r;
          o[plane_px + i] = (uint8_t)g;
          o[2 * plane_px + i] = (uint8_t)b;
        }
      }
    }
    if (V16) {
      *reinterpret_cast<u32x4*>(o) = (u32x4){pr[0], pr[1], pr[2], pr[3]};
      *reinterpret_cast<u32x4*>(o + plane_px) = (u32x4){pg[0], pg[1], pg[2], pg[3]};
      *reinterpret_cast<u32x4*>(o + 2 * plane_px) = (u32x4){pb[0], pb[1], pb[2], pb[3]};
    }
  }
}

// Dynamic LDS of one workgroup: the planes as the kernel lays them out, 8 VS luma rows and per chroma plane 8 rows plus the
// 4:2:0 halo rows, ypitch = 8 * (luma block columns), cpitch = 8 * (chroma block columns).  The columns are the kernel's:
// the whole padded MCU grid (bw0 = mcus_x * HS, mcus_x) without a window, jc_window's with one.  For 2:1 chroma the padded
// grid can be one luma block column wider than the frame (W % 16 in 1..8), which the full window's ceil(W / 8) is not.
static long jpeg_pixels_lds_bytes(const JcGeom& g, const JcWindow* win) {
  const int halo = g.samp == JC_420 ? 1 : 0, nc = g.samp == JC_GREY ? 0 : 2;
  const int ybx_n = win ? win->ybx_n : g.bw[0], cbx_n = win ? win->cbx_n : g.mcus_x;
  return 8L * g.vs * ybx_n * 8 + (long)nc * (8 + 2 * halo) * cbx_n * 8;
}

// dst_row == nullptr: the identity-row instance (tdeed_jpeg_pixels); win: the window of tdeed_jpeg_pixels_window, nullptr for
// the whole frame.  out holds (h, w) planes, the window's size or the frame's.
template <int SAMP>
static int jpeg_pixels_launch(const int16_t* coef, const int* frame_set, const uint8_t* sets, int n_sets, uint8_t* out,
                              const int* dst_row, long out_rows, int frame_lo, int n_frames, int H, int W, const JcWindow* win,
                              hipStream_t st) {
  const JcGeom g = jc_geom(W, H, SAMP);
  const JcWindow w = win ? *win : jc_window(g, 0, 0, H, W);
  const long lds = jpeg_pixels_lds_bytes(g, win);
  TD_CHECK(lds <= 64 * 1024, "jpeg_pixels: a band of a %d pixel wide frame needs %ld bytes of LDS (limit 65536)", w.ww, lds);
  TD_CHECK(g.mcus_y <= 65535 && n_frames <= 65535, "jpeg_pixels: %d bands x %d frames exceed the grid", g.mcus_y, n_frames);
  const bool v16 = w.ww % 16 == 0 && (((uintptr_t)out) & 15) == 0;
  const dim3 grid(w.band_n, n_frames);
#define JPEG_PIXELS_GO(V16, ROWS, WIN)                                                                                              \
  hipLaunchKernelGGL((jpeg_pixels_kernel<SAMP, V16, ROWS, WIN>), grid, dim3(256), lds, st, coef, frame_set, (const JcTableSet*)sets, \
                     n_sets, frame_lo, W, H, g.mcus_x, g.mcus_y, out, dst_row, out_rows, w)
  if (win) {
    if (v16) JPEG_PIXELS_GO(true, true, true); else JPEG_PIXELS_GO(false, true, true);
  } else if (dst_row) {
    if (v16) JPEG_PIXELS_GO(true, true, false); else JPEG_PIXELS_GO(false, true, false);
  } else {
    if (v16) JPEG_PIXELS_GO(true, false, false); else JPEG_PIXELS_GO(false, false, false);
  }
#undef JPEG_PIXELS_GO
  TD_LAUNCH_CHECK("jpeg_pixels");
  return TDEED_OK;
}

static int jpeg_pixels_any(const int16_t* coeff, const int* frame_table_set, const uint8_t* table_sets, int n_sets, uint8_t* out,
                           const int* dst_row, long out_rows, int frame_lo, int n_frames, int H, int W, int sampling,
                           const JcWindow* win, void* hip_stream) {
  TD_CHECK(coeff && frame_table_set && table_sets && out, "jpeg_pixels: null pointer");
  TD_CHECK(n_sets > 0 && n_frames > 0 && frame_lo >= 0, "jpeg_pixels: bad sizes");
  TD_CHECK(W > 0 && H > 0 && W <= 65535 && H <= 65535, "jpeg_pixels: bad frame size %dx%d", H, W);
  TD_CHECK((((uintptr_t)table_sets | (uintptr_t)coeff) & 15) == 0 && (((uintptr_t)frame_table_set) & 3) == 0,
           "jpeg_pixels: table sets and coefficients must be 16-byte aligned");
  hipStream_t st = (hipStream_t)hip_stream;
  switch (sampling) {
    case JC_GREY:
      return jpeg_pixels_launch<JC_GREY>(coeff, frame_table_set, table_sets, n_sets, out, dst_row, out_rows, frame_lo, n_frames, H, W,
                                         win, st);
    case JC_444:
      return jpeg_pixels_launch<JC_444>(coeff, frame_table_set, table_sets, n_sets, out, dst_row, out_rows, frame_lo, n_frames, H, W,
                                         win, st);
    case JC_422:
      return jpeg_pixels_launch<JC_422>(coeff, frame_table_set, table_sets, n_sets, out, dst_row, out_rows, frame_lo, n_frames, H, W,
                                         win, st);
    case JC_420:
      return jpeg_pixels_launch<JC_420>(coeff, frame_table_set, table_sets, n_sets, out, dst_row, out_rows, frame_lo, n_frames, H, W,
                                         win, st);
  }
  TD_CHECK(false, "jpeg_pixels: sampling %d (0 grey, 1 4:4:4, 2 4:2:2, 3 4:2:0)", sampling);
  return TDEED_OK;
}

extern "C" int tdeed_jpeg_pixels(const int16_t* coeff, const int* frame_table_set, const uint8_t* table_sets, int n_sets,
                                 uint8_t* out, int frame_lo, int n_frames, int H, int W, int sampling, void* hip_stream) {
  return jpeg_pixels_any(coeff, frame_table_set, table_sets, n_sets, out, nullptr, 0, frame_lo, n_frames, H, W, sampling, nullptr,
                         hip_stream);
}

extern "C" int tdeed_jpeg_pixels_rows(const int16_t* coeff, const int* frame_table_set, const uint8_t* table_sets, int n_sets,
                                      uint8_t* out, long out_rows, const int* dst_row, int frame_lo, int n_frames, int H, int W,
                                      int sampling, void* hip_stream) {
  TD_CHECK(dst_row && (((uintptr_t)dst_row) & 3) == 0, "jpeg_pixels_rows: dst_row must be a 4-byte aligned device pointer");
  TD_CHECK(out_rows > 0, "jpeg_pixels_rows: out_rows %ld", out_rows);
  return jpeg_pixels_any(coeff, frame_table_set, table_sets, n_sets, out, dst_row, out_rows, frame_lo, n_frames, H, W, sampling,
                         nullptr, hip_stream);
}

// tdeed_jpeg_pixels_rows over the window [top, top + wh) x [left, left + ww) of the H x W frames: out holds rows of (3, wh, ww)
extern "C" int tdeed_jpeg_pixels_window(const int16_t* coeff, const int* frame_table_set, const uint8_t* table_sets, int n_sets,
                                        uint8_t* out, long out_rows, const int* dst_row, int frame_lo, int n_frames, int H, int W,
                                        int sampling, int top, int left, int wh, int ww, void* hip_stream) {
  TD_CHECK(dst_row && (((uintptr_t)dst_row) & 3) == 0, "jpeg_pixels_window: dst_row must be a 4-byte aligned device pointer");
  TD_CHECK(out_rows > 0, "jpeg_pixels_window: out_rows %ld", out_rows);
  TD_CHECK(W > 0 && H > 0 && W <= 65535 && H <= 65535, "jpeg_pixels_window: bad frame size %dx%d", H, W);
  TD_CHECK(sampling >= JC_GREY && sampling <= JC_420, "jpeg_pixels_window: sampling %d (0 grey, 1 4:4:4, 2 4:2:2, 3 4:2:0)", sampling);
  TD_CHECK(top >= 0 && left >= 0 && wh > 0 && ww > 0 && wh <= H - top && ww <= W - left,
           "jpeg_pixels_window: the window %dx%d at (%d, %d) is empty or leaves the %dx%d frame", wh, ww, top, left, H, W);
  const JcWindow w = jc_window(jc_geom(W, H, sampling), top, left, wh, ww);
  return jpeg_pixels_any(coeff, frame_table_set, table_sets, n_sets, out, dst_row, out_rows, frame_lo, n_frames, H, W, sampling, &w,
                         hip_stream);
}

// the dynamic LDS bytes the launchers request per workgroup: of tdeed_jpeg_pixels / tdeed_jpeg_pixels_rows when windowed == 0
// (the window arguments are ignored), of tdeed_jpeg_pixels_window otherwise; -1 for a bad geometry or window
extern "C" long tdeed_jpeg_pixels_lds_bytes(int W, int H, int sampling, int windowed, int top, int left, int wh, int ww) {
  if (W <= 0 || H <= 0 || W > 65535 || H > 65535 || sampling < JC_GREY || sampling > JC_420) return -1;
  const JcGeom g = jc_geom(W, H, sampling);
  if (!windowed) return jpeg_pixels_lds_bytes(g, nullptr);
  if (top < 0 || left < 0 || wh <= 0 || ww <= 0 || wh > H - top || ww > W - left) return -1;
  const JcWindow w = jc_window(g, top, left, wh, ww);
  return jpeg_pixels_lds_bytes(g, &w);
}

// the ranges of jc_window as ten ints (jpegdev.window_blocks is held against them): band_lo, band_n, ybx_lo, ybx_n, ybr_lo,
// ybr_hi, cbx_lo, cbx_n, mrow_lo, mrow_hi; -1 for a bad geometry or window
extern "C" int tdeed_jpeg_window_blocks(int W, int H, int sampling, int top, int left, int wh, int ww, int* ranges) {
  if (!ranges || W <= 0 || H <= 0 || W > 65535 || H > 65535 || sampling < JC_GREY || sampling > JC_420) return -1;
  if (top < 0 || left < 0 || wh <= 0 || ww <= 0 || wh > H - top || ww > W - left) return -1;
  const JcWindow w = jc_window(jc_geom(W, H, sampling), top, left, wh, ww);
  const int r[10] = {w.band_lo, w.band_n, w.ybx_lo, w.ybx_n, w.ybr_lo, w.ybr_hi, w.cbx_lo, w.cbx_n, w.mrow_lo, w.mrow_hi};
  for (int i = 0; i < 10; ++i) ranges[i] = r[i];
  return 0;
}
