// Host check of the piece decode of t-deed_amd/csrc/jpeg_core.h: every segment of a packed video is walked once with the
// recording instance of jc_entropy_run (the index pass of csrc/jpeg.hip), then every recorded piece is decoded on its own
// into a fresh zero buffer, as the lanes of tdeed_jpeg_entropy_items do.  The union of the pieces must be what the
// whole-segment decode gives; the caller compares.  No GPU; meant to run under host sanitizers as well.
//
//   c++ -O2 -std=c++17 -o jpeg_split_check tools/jpeg_split_check.cpp
//   jpeg_split_check packed.bin split_mcus out.bin          (split_mcus 0: one MCU row)
//
// packed.bin: the format of tdeed_amd.jpegdev.PackedJpegs.save (see tools/jpeg_host_check.cpp).
// out.bin: int32 n_pieces, int16 whole-segment coefficients [frames][frame_blocks * 64], int32 whole-segment status
//   [segments], int16 coefficients of the pieces' union [frames][frame_blocks * 64], int32 piece status [n_pieces],
//   int32 pieces per segment [segments], int32 index-pass status [segments], int32 overlaps (values two pieces both set),
//   the piece rows [n_pieces][72] (JcPiece; pos counts from the start of the packed stream).
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
  if (argc != 4) {
    fprintf(stderr, "usage: %s packed.bin split_mcus out.bin\n", argv[0]);
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
  if (W <= 0 || H <= 0 || W > 65535 || H > 65535 || samp < JC_GREY || samp > JC_420 || n_frames < 0 || n_seg < 0 || n_sets < 0 ||
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
  const long frame_coefs = (long)g.frame_blocks * 64;
  std::vector<int16_t> whole(frame_coefs * n_frames, 0), joined(frame_coefs * n_frames, 0);
  std::vector<int32_t> status(n_seg, 0), index_status(n_seg, 0), per_seg(n_seg, 0), piece_status;
  std::vector<JcPiece> pieces;
  int32_t overlaps = 0;
  for (int i = 0; i < n_seg; ++i) {
    const JcSegment& s = segs[i];
    if (!jc_segment_ok(s, stream_bytes, n_sets, total_mcus) || s.frame < 0 || s.frame >= n_frames) {
      status[i] = index_status[i] = JC_ERR_TABLE;
      continue;
    }
    // the segment alone in an exact-size heap block: a read outside [offset, offset + length) is an error the sanitizer sees
    std::vector<uint8_t> own(stream.begin() + s.offset, stream.begin() + s.offset + s.length);
    status[i] = jc_entropy_segment(own.data(), s.length, s.first_mcu, s.n_mcu, &sets[s.set], samp, g.mcus_x, g.mcus_y,
                                   whole.data() + (long)s.frame * frame_coefs);
    // the index pass: the first piece starts where the segment does, the recorder adds one per split point passed
    const size_t row0 = pieces.size();
    Recorder rec;
    rec.rows = &pieces;
    rec.seg_len = s.length; rec.end_mcu = s.first_mcu + s.n_mcu; rec.split = split;
    JcPiece& p = rec.proto;
    memset(&p, 0, sizeof p);
    p.pos = s.offset; p.segment = i; p.set = s.set;
    const JcState zero = jc_zero_state();
    rec(s.first_mcu, zero);
    index_status[i] = jc_entropy_run<false>(own.data(), s.length, zero, s.first_mcu, s.n_mcu, &sets[s.set], samp, g.mcus_x,
                                            g.mcus_y, (int16_t*)nullptr, split, rec);
    per_seg[i] = (int32_t)(pieces.size() - row0);
    if (index_status[i] == JC_OK && per_seg[i] != jc_piece_count(s.first_mcu, s.n_mcu, split)) {
      fprintf(stderr, "segment %d: %d pieces recorded, the rule says %d\n", i, per_seg[i], jc_piece_count(s.first_mcu, s.n_mcu, split));
      return 3;
    }
    // every piece on its own: its bytes alone in an exact-size block, its coefficients in a fresh zero frame
    for (size_t k = row0; k < pieces.size(); ++k) {
      const JcPiece& q = pieces[k];
      if (!jc_piece_ok(q, stream_bytes, n_sets, total_mcus)) {
        piece_status.push_back(JC_ERR_TABLE);
        continue;
      }
      std::vector<uint8_t> bytes(stream.begin() + q.pos, stream.begin() + q.pos + q.left);
      std::vector<int16_t> fresh(frame_coefs, 0);
      JcNoRecord none;
      piece_status.push_back(jc_entropy_run<true>(bytes.data(), q.left, q.st, q.first_mcu, q.n_mcu, &sets[q.set], samp, g.mcus_x,
                                                  g.mcus_y, fresh.data(), 1, none));
      int16_t* dst = joined.data() + (long)s.frame * frame_coefs;
      for (long v = 0; v < frame_coefs; ++v)
        if (fresh[v]) {
          overlaps += dst[v] != 0;
          dst[v] = fresh[v];
        }
    }
  }

  FILE* o = fopen(argv[3], "wb");
  if (!o) {
    perror(argv[3]);
    return 2;
  }
  const int32_t n_pieces = (int32_t)pieces.size();
  fwrite(&n_pieces, sizeof n_pieces, 1, o);
  fwrite(whole.data(), sizeof(int16_t), whole.size(), o);
  fwrite(status.data(), sizeof(int32_t), n_seg, o);
  fwrite(joined.data(), sizeof(int16_t), joined.size(), o);
  fwrite(piece_status.data(), sizeof(int32_t), piece_status.size(), o);
  fwrite(per_seg.data(), sizeof(int32_t), n_seg, o);
  fwrite(index_status.data(), sizeof(int32_t), n_seg, o);
  fwrite(&overlaps, sizeof overlaps, 1, o);
  fwrite(pieces.data(), sizeof(JcPiece), pieces.size(), o);
  fclose(o);
  int bad = 0;
  for (int i = 0; i < n_seg; ++i) bad += status[i] != 0;
  printf("%d frames, %d segments, %d pieces of %d MCUs, %d segments with errors\n", n_frames, n_seg, n_pieces, split, bad);
  return 0;
}
