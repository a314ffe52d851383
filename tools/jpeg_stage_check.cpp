// Host check of the relocated piece decode of t-deed_amd/csrc/jpeg_core.h (jc_reloc_ok / jc_piece_reloc_ok, the rule of
// tdeed_jpeg_entropy_items_reloc): the packed stream of a video is indexed once, its piece rows carrying positions in a
// numbering that starts far above the stream (as the rows of a streamed shard do), then the stream is cut into ranges at
// segment boundaries, each range starting at a multiple of 16, and every range is copied into a heap block of exactly
// `shift` + its size -- the staged copy.  Every piece is decoded from its range's block through the relocation predicate and
// must give the coefficients of the whole-stream decode; relocation rows that leave the window or the block must all be
// rejected, and the tightest window must be accepted.  No GPU; meant to run under host sanitizers: a read outside a staged
// copy is a read outside its heap block.
//
//   c++ -O2 -std=c++17 -o jpeg_stage_check tools/jpeg_stage_check.cpp
//   jpeg_stage_check packed.bin split_mcus n_ranges shift        (split_mcus 0: one MCU row; shift: a multiple of 16)
//
// packed.bin: the format of tdeed_amd.jpegdev.PackedJpegs.save (see tools/jpeg_host_check.cpp).
// Prints "pieces P ranges R decoded D rejected J accepted_tight A"; exit status 3 when a decode differs from the whole-stream
// decode, a row that must be rejected passes, or a tight window is refused.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../t-deed_amd/csrc/jpeg_core.h"

struct Recorder {
  static constexpr bool on = true;
  std::vector<JcPiece>* rows;
  JcPiece proto;
  int seg_len, end_mcu, split;
  void operator()(int m, const JcState& st) {
    JcPiece p = proto;
    p.pos = proto.pos + st.byte_off;
    p.first_mcu = m;
    const int to_next = split - m % split;
    p.n_mcu = to_next < end_mcu - m ? to_next : end_mcu - m;
    p.left = seg_len - st.byte_off;
    p.st = st;
    rows->push_back(p);
  }
};

static bool read_all(FILE* f, void* dst, size_t n) { return n == 0 || fread(dst, 1, n, f) == n; }

int main(int argc, char** argv) {
  if (argc != 5) {
    fprintf(stderr, "usage: %s packed.bin split_mcus n_ranges shift\n", argv[0]);
    return 2;
  }
  FILE* f = fopen(argv[1], "rb");
  if (!f) {
    perror(argv[1]);
    return 2;
  }
  int32_t hdr[8];
  if (!read_all(f, hdr, sizeof hdr) || hdr[0] != 0x314B504A) {
    fprintf(stderr, "%s: not a packed video\n", argv[1]);
    return 2;
  }
  const int W = hdr[1], H = hdr[2], samp = hdr[3], n_frames = hdr[4], n_seg = hdr[5], n_sets = hdr[6];
  const long stream_bytes = hdr[7];
  if (W <= 0 || H <= 0 || W > 65535 || H > 65535 || samp < JC_GREY || samp > JC_420 || n_frames < 0 || n_seg <= 0 || n_sets < 0 ||
      stream_bytes < 0) {
    fprintf(stderr, "%s: bad header\n", argv[1]);
    return 2;
  }
  std::vector<int32_t> frame_set(n_frames);
  std::vector<JcSegment> segs(n_seg);
  std::vector<JcTableSet> sets(n_sets);
  std::vector<uint8_t> stream(stream_bytes);
  if (!read_all(f, frame_set.data(), sizeof(int32_t) * n_frames) || !read_all(f, segs.data(), sizeof(JcSegment) * n_seg) ||
      !read_all(f, sets.data(), sizeof(JcTableSet) * n_sets) || !read_all(f, stream.data(), stream_bytes)) {
    fprintf(stderr, "%s: truncated\n", argv[1]);
    return 2;
  }
  fclose(f);
  const JcGeom g = jc_geom(W, H, samp);
  const int total_mcus = g.mcus_x * g.mcus_y;
  int split = atoi(argv[2]);
  if (split <= 0) split = g.mcus_x;
  int n_ranges = atoi(argv[3]);
  const long shift = atol(argv[4]);
  if (n_ranges < 1 || shift < 0 || shift % 16) {
    fprintf(stderr, "n_ranges must be positive, shift a non-negative multiple of 16\n");
    return 2;
  }
  if (n_ranges > n_seg) n_ranges = n_seg;
  const long frame_coefs = (long)g.frame_blocks * 64;
  const int64_t vbase = ((int64_t)1 << 33) + 4096;              // the shard's place in the set-wide numbering of JcPiece.pos

  // the whole-stream decode and the index pass, as tools/jpeg_split_check.cpp runs them
  std::vector<int16_t> whole(frame_coefs * n_frames, 0), joined(frame_coefs * n_frames, 0);
  std::vector<JcPiece> pieces;
  for (int i = 0; i < n_seg; ++i) {
    const JcSegment& s = segs[i];
    if (!jc_segment_ok(s, stream_bytes, n_sets, total_mcus) || s.frame < 0 || s.frame >= n_frames) {
      fprintf(stderr, "segment %d: bad row\n", i);
      return 2;
    }
    if (jc_entropy_segment(stream.data() + s.offset, s.length, s.first_mcu, s.n_mcu, &sets[s.set], samp, g.mcus_x, g.mcus_y,
                           whole.data() + (long)s.frame * frame_coefs) != JC_OK) {
      fprintf(stderr, "segment %d: the whole-stream decode fails\n", i);
      return 2;
    }
    Recorder rec;
    rec.rows = &pieces;
    rec.seg_len = s.length; rec.end_mcu = s.first_mcu + s.n_mcu; rec.split = split;
    JcPiece& p = rec.proto;
    memset(&p, 0, sizeof p);
    p.pos = vbase + s.offset; p.segment = i; p.set = s.set;
    const JcState zero = jc_zero_state();
    rec(s.first_mcu, zero);
    jc_entropy_run<false>(stream.data() + s.offset, s.length, zero, s.first_mcu, s.n_mcu, &sets[s.set], samp, g.mcus_x, g.mcus_y,
                          (int16_t*)nullptr, split, rec);
  }

  // the ranges: runs of segment rows (laid out in row order), from the first row's byte rounded down to 16 to the last row's end
  struct Range {
    long lo16, hi;
    std::vector<uint8_t> block;                                  // `shift` bytes, then the copy: exactly what was staged
    JcReloc rel;
  };
  std::vector<Range> ranges(n_ranges);
  std::vector<int> seg_range(n_seg);
  for (int r = 0; r < n_ranges; ++r) {
    const int a = (int)((long)r * n_seg / n_ranges), b = (int)((long)(r + 1) * n_seg / n_ranges);
    Range& R = ranges[r];
    R.lo16 = segs[a].offset & ~15L;
    R.hi = 0;
    for (int i = a; i < b; ++i) {
      seg_range[i] = r;
      const long end = (long)segs[i].offset + segs[i].length;
      R.hi = end > R.hi ? end : R.hi;
      if (segs[i].offset < R.lo16) {
        fprintf(stderr, "segment %d lies before its range: the rows are not in byte order\n", i);
        return 2;
      }
    }
    R.block.assign(shift, 0xFF);
    R.block.insert(R.block.end(), stream.begin() + R.lo16, stream.begin() + R.hi);
    R.rel.delta = vbase + R.lo16 - shift;
    R.rel.lo = shift;
    R.rel.hi = shift + (R.hi - R.lo16);
    if (R.rel.delta % 16) return 3;
  }

  int decoded = 0, rejected = 0, must_reject = 0, tight = 0, failures = 0;
  for (const JcPiece& q : pieces) {
    const Range& R = ranges[seg_range[q.segment]];
    const long block_bytes = (long)R.block.size();
    if (!jc_piece_reloc_ok(q, R.rel, block_bytes, n_sets, total_mcus)) {
      fprintf(stderr, "piece of segment %d: refused in its own range\n", q.segment);
      ++failures;
      continue;
    }
    std::vector<int16_t> fresh(frame_coefs, 0);
    JcNoRecord none;
    const int st = jc_entropy_run<true>(R.block.data() + (q.pos - R.rel.delta), q.left, q.st, q.first_mcu, q.n_mcu, &sets[q.set], samp,
                                        g.mcus_x, g.mcus_y, fresh.data(), 1, none);
    failures += st != JC_OK;
    ++decoded;
    int16_t* dst = joined.data() + (long)segs[q.segment].frame * frame_coefs;
    for (long v = 0; v < frame_coefs; ++v)
      if (fresh[v]) dst[v] = fresh[v];
    // rows that must be rejected, and the tightest one that must pass
    const int64_t at = q.pos - R.rel.delta;                      // where the piece starts in the block
    JcReloc t = R.rel;
    t.lo = at; t.hi = at + q.left;
    if (jc_piece_reloc_ok(q, t, block_bytes, n_sets, total_mcus)) ++tight; else ++failures;
    std::vector<JcReloc> bad;
    t = R.rel; t.lo = at + 1; bad.push_back(t);                  // the piece starts before its window
    if (q.left > 0) { t = R.rel; t.hi = at + q.left - 1; bad.push_back(t); }   // ... ends behind it
    t = R.rel; t.delta = q.pos + 1; t.lo = 0; bad.push_back(t);  // a relocation that points before the buffer
    t = R.rel; t.delta = R.rel.delta + block_bytes + 16; bad.push_back(t);     // ... far before it
    t = R.rel; t.delta = R.rel.delta - block_bytes - 16; t.hi = block_bytes; bad.push_back(t);   // behind the buffer
    t = R.rel; t.hi = block_bytes + 1; bad.push_back(t);         // a window that leaves the buffer
    t = R.rel; t.lo = -16; bad.push_back(t);
    t = R.rel; t.lo = R.rel.hi; t.hi = R.rel.lo; bad.push_back(t);             // an inverted window
    t = R.rel; t.delta = INT64_MIN; bad.push_back(t);            // nothing overflows
    t = R.rel; t.delta = INT64_MAX; bad.push_back(t);
    for (const JcReloc& b : bad) {
      ++must_reject;
      if (jc_piece_reloc_ok(q, b, block_bytes, n_sets, total_mcus)) ++failures; else ++rejected;
    }
    JcPiece neg = q;
    neg.left = -1;
    ++must_reject;
    if (jc_piece_reloc_ok(neg, R.rel, block_bytes, n_sets, total_mcus)) ++failures; else ++rejected;
    neg = q;
    neg.pos = -q.pos;
    ++must_reject;
    if (jc_piece_reloc_ok(neg, R.rel, block_bytes, n_sets, total_mcus)) ++failures; else ++rejected;
  }
  if (memcmp(whole.data(), joined.data(), sizeof(int16_t) * whole.size()) != 0) {
    fprintf(stderr, "the staged decode differs from the whole-stream decode\n");
    ++failures;
  }
  printf("pieces %d ranges %d decoded %d rejected %d accepted_tight %d\n", (int)pieces.size(), n_ranges, decoded, rejected, tight);
  if (rejected != must_reject) ++failures;
  return failures ? 3 : 0;
}
