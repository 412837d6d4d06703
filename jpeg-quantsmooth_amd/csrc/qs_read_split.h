// qs_read_split.h -- the split route of the device scan reader (qs_hip_read_split_device_batch,
// csrc/qs_kernels_read_split.hip): what its kernels, the host driver (csrc/qs_read_job.cpp) and a plain host build
// (tests/read_split_host.cpp) share.  Same input and same output as qs_read.h; DESIGN.md section 14.
//
// Every restart interval -- the whole scan when the file has no markers -- is cut into segments of QS_RD_SPLIT_BYTES
// stuffed bytes, and one lane decodes one segment.  The first segment of an interval enters in the known state; every
// other one starts from a guess (byte aligned, a DC symbol next, block 0 of the table period) and takes, in each of
// QS_RD_SPLIT_ROUNDS further launches, the state its left neighbour left in the launch before.  Huffman streams
// synchronise themselves, so after a few rounds every entry is its neighbour's exit; that is then CHECKED link by link:
// the first entry is true, each lane decoded from its entry, so by induction every entry is true.  A job with a broken
// link gets status 4.  The DC predictions are rebuilt from the differences by a prefix sum.
//
// The state between two symbols is (bit position in the stuffed stream, k, u mod p): k the zigzag index (0: the DC
// symbol is next), u the block of the MCU and p the smallest period of the table pairs (Td, Ta) over an MCU's blocks.
// u itself is NOT part of it: with equal tables two decoders that differ only in u would never agree.  The true block
// index of a segment's first block comes from a prefix sum of the blocks each segment completed.
//
// Bounds, for every function here:
//   * per launch a lane reads bytes [its entry, its segment's end) and the rest of one symbol: at most
//     QS_RD_SPLIT_BYTES + 1 bytes and 31 bits with their stuffing; an entry in front of the lane's own segment (a chain
//     that cannot go on) decodes nothing;
//   * the byte cursor never passes the interval's end (QrBits.end); a symbol that would take bits from behind it is
//     not decoded;
//   * the symbol loop is bounded by QS_RD_SPLIT_BYTES * 8 + 64 (a symbol takes at least one bit), the other loops over
//     decoded data by 8 bytes per refill, code lengths 9..16 and 63 coefficients;
//   * the write pass checks the block index against the interval's own block count before it touches a block, the
//     coefficient index against the array's stride and size before every store.
#pragma once
#include "qs_read.h"

#ifndef QS_RD_SPLIT_BYTES
#define QS_RD_SPLIT_BYTES 256      // B: stuffed bytes per segment
#endif
#ifndef QS_RD_SPLIT_ROUNDS
#define QS_RD_SPLIT_ROUNDS 17      // R: synchronisation launches (twice the 8 the worst file of the corpus needs, plus one)
#endif
#define QS_RD_SPLIT_WG 256         // lanes per workgroup of every split kernel (= segments, = MCUs of a scan tile)
#define QS_RD_NOSYNC 4             // d_status: an entry still differed from its neighbour's exit after R rounds

// One job's part of the workspace beyond QrJob (which the marker kernels take as it is)
struct QrsJob {
  int32_t period;                  // p
  int32_t pad;
  uint8_t dct[12], act[12];        // block u of an MCU: its tables tab[dct[u]] / tab[4 + act[u]] ...
  uint8_t comp[12], bx[12], by[12];  // ... its component and its place inside the MCU
  uint64_t max_segments;           // no scan of this geometry has more
  uint64_t off_nseg;               // uint32: segments of this run (0: status 1, nothing to decode)
  uint64_t off_seg0;               // uint32[intervals + 1]: the first segment of each interval
  uint64_t off_entry;              // uint64[max_segments]: the state each lane decoded from last
  uint64_t off_exit;               // uint64[2][max_segments]: the state it reached, double-buffered over the rounds
  uint64_t off_cnt;                // uint32[max_segments]: the blocks it completed
  uint64_t off_stile;              // uint32[segment tiles][2] (blocks behind the tile's last interval start, whether
                                   // it holds one), then uint32[segment tiles]: the blocks in front of each tile
  uint64_t off_dcd;                // int16[nblocks]: the DC differences in scan order
  uint64_t off_mtile;              // uint32[MCU tiles][5] (4 sums and the flag), then uint32[MCU tiles][4]
};

// the pointers of one job (device: from the offsets; host: vectors)
struct QrsBufs {
  uint32_t* nseg;
  uint32_t* seg0;
  uint64_t* entry;
  uint64_t* exit[2];
  uint32_t* cnt;
  int16_t* dcd;
};

QS_RD_HD uint64_t qrs_max_segments(uint64_t max_scan, int intervals) {
  return max_scan / QS_RD_SPLIT_BYTES + (uint64_t)intervals + 1;
}

// the blocks of an MCU in scan order and the period of their table pairs
QS_RD_HD void qrs_describe(const QrJob& J, QrsJob* S) {
  int u = 0;
  for (int c = 0; c < J.g.ncomp && c < 4; ++c)
    for (int kk = 0; kk < J.g.hs[c] * J.g.vs[c] && u < 10; ++kk, ++u) {
      S->comp[u] = (uint8_t)c;
      S->by[u] = (uint8_t)(kk / J.g.hs[c]);
      S->bx[u] = (uint8_t)(kk % J.g.hs[c]);
      S->dct[u] = (uint8_t)(J.dc_tbl[c] & 3);
      S->act[u] = (uint8_t)(J.ac_tbl[c] & 3);
    }
  int p = 1;
  for (; p < u; ++p) {
    if (u % p) continue;
    bool same = true;
    for (int i = p; i < u; ++i) same = same && S->dct[i] == S->dct[i - p] && S->act[i] == S->act[i - p];
    if (same) break;
  }
  S->period = p;
}

// ---- the state -------------------------------------------------------------------------------------------------------------

QS_RD_HD uint64_t qrs_pack(uint64_t bitpos, int k, int um) { return (bitpos << 12) | ((uint64_t)k << 4) | (uint64_t)um; }

// qr_fill that remembers, one bit per byte it loaded, whether a stuffed 00 was dropped behind the byte
QS_RD_HD void qrs_fill(QrBits& b, uint32_t& ff) {
  for (int i = 0; i < 8 && b.left <= 56; ++i) {
    uint32_t c = 0, skipped = 0;
    if (b.pos < b.end) {
      const int64_t d = (int64_t)b.pos - b.win0;
      if (d < 0 || d >= 8) b.win = qr_unit8(b.s, b.pos, &b.win0);
      c = (uint32_t)(b.win >> (8 * ((int64_t)b.pos - b.win0))) & 0xFF;
      ++b.pos;
      if (c == 0xFF && b.pos < b.end) {
        ++b.pos;
        skipped = 1;
      }
    } else {
      b.pad += 8;
    }
    ff = (ff << 1) | skipped;
    b.buf = (b.buf << 8) | c;
    b.left += 8;
  }
}

// where the next unread bit lies in the stuffed stream, in bits; the interval's end when nothing of it is unread.  The
// byte is never the 00 behind an FF.
QS_RD_HD uint64_t qrs_pos(const QrBits& b, uint32_t ff) {
  const int real = b.left - b.pad;
  if (real <= 0) return b.end * 8;
  const int nb = (real + 7) >> 3;                                  // bytes that hold unread bits, at most 8
  const uint32_t m = (ff >> (b.pad >> 3)) & ((1u << nb) - 1u);
  return (b.pos - (uint64_t)nb - (uint64_t)__builtin_popcount(m)) * 8 + (uint64_t)((8 - (real & 7)) & 7);
}

// the byte segment s of interval [start, end) begins at: never the 00 of an FF 00 pair
QS_RD_HD uint64_t qrs_bound(const QrSrc& src, uint64_t start, uint64_t end, uint64_t s) {
  uint64_t p = start + s * QS_RD_SPLIT_BYTES;
  if (p >= end) return end;
  if (s > 0 && qr_byte(src, p - 1) == 0xFF && qr_byte(src, p) == 0) ++p;
  return p;
}

QS_RD_HD uint64_t qrs_segments(uint64_t start, uint64_t end) {
  const uint64_t n = (end - start + QS_RD_SPLIT_BYTES - 1) / QS_RD_SPLIT_BYTES;
  return n ? n : 1;                                                // (an empty interval is still somebody's to report)
}

// ---- one segment -------------------------------------------------------------------------------------------------------------

// what the write pass needs beyond the walk itself
struct QrsSink {
  const QsEncGeom* g;
  QrOut out;
  int16_t* dcd;                    // the job's DC differences in scan order
  long long blk0;                  // scan-order index of the interval's first block
  long long nblk;                  // blocks of the interval: nothing is stored for a block at or behind it
  long long bi;                    // the block the entry lies in, counted inside the interval
  int status;                      // <- QS_RD_OK / QS_RD_LENGTH / QS_RD_CODE
};

// a[i] of four, without an indexed private array (which would live in scratch on the device)
template <class T> QS_RD_HD T qrs_pick4(const T* a, int i) { return i == 0 ? a[0] : i == 1 ? a[1] : i == 2 ? a[2] : a[3]; }

QS_RD_HD int16_t* qrs_block(const QrsJob& S, const QrsSink& w, long long bi) {
  const QsEncGeom& g = *w.g;
  const long long gi = w.blk0 + bi;
  const int m = (int)(gi / g.bpm), u = (int)(gi - (long long)m * g.bpm);
  const int c = S.comp[u], slot = g.slot[c] & 3, stride = g.stride[c];
  const int my = m / g.mcus_x, mx = m - my * g.mcus_x;
  const int bx = mx * g.hs[c] + S.bx[u], by = my * g.vs[c] + S.by[u];
  const long long idx = (long long)by * stride + bx;
  return (bx < stride && idx < qrs_pick4(w.out.nblk, slot)) ? qrs_pick4(w.out.coef, slot) + idx * 64 : nullptr;
}

// Symbols from `entry` while they start in front of byte `hi` (<= iend, the interval's end) and lie wholly inside the
// interval.  -> *exit: the state in front of the first symbol that was not decoded; *cnt: the blocks completed.
// W false: nothing but that; bits without a code, or a run that passes coefficient 63, put k back to 0 (and skip one
// bit where no symbol was taken) -- on a guessed entry that is no error.  W true (every entry proved true): non-zero AC
// values and DC differences are stored; the walk ends with w->status QS_RD_CODE on such bits, and behind the interval's
// last block, where it checks what is left of the interval as qr_decode_interval does.
template <bool W>
QS_RD_HD void qrs_walk(const QrTable* tab, const QrsJob& S, const QrSrc& src, uint64_t iend, uint64_t lo, uint64_t hi,
                       uint64_t entry, uint64_t* exit, uint32_t* cnt, QrsSink* w) {
  static constexpr uint8_t zz[64] = QS_RD_ZZ_INIT;
  const uint64_t byte0 = entry >> 15;
  int k = (int)(entry >> 4) & 127, um = (int)entry & 15;
  *exit = entry;
  *cnt = 0;
  // a true entry lies in the lane's own segment; one in front of it is a chain that could not go on, and stays
  if (byte0 < lo || byte0 >= iend || k > 63 || um >= S.period) return;
  if (W && w->bi >= w->nblk) return;
  QrBits b;
  uint32_t ff = 0, done = 0;
  qr_bits_init(b, src, byte0, iend);
  qrs_fill(b, ff);
  b.left -= (int)(entry >> 12) & 7;
  int16_t* blk = nullptr;
  if (W) blk = qrs_block(S, *w, w->bi);
  uint64_t p = entry >> 12;
  for (int it = 0; it < QS_RD_SPLIT_BYTES * 8 + 64; ++it) {
    if (b.left < 32) qrs_fill(b, ff);
    p = qrs_pos(b, ff);
    if (p >= hi * 8) break;
    const int left0 = b.left;
    const int sym = qr_symbol(b, k == 0 ? tab[S.dct[um]] : tab[4 + S.act[um]]);
    if (sym < 0) {
      if (left0 - b.pad < 16) break;                               // (the zeros behind the interval may be to blame)
      if (W) {
        w->status = QS_RD_CODE;
        break;
      }
      b.left = left0 - 1;
      k = 0;
      continue;
    }
    const int s = sym & 15;
    uint32_t r = 0;
    if (s) {
      r = qr_peek(b, s);
      b.left -= s;
    }
    if (b.left < b.pad) {                                          // it ends behind the interval: not decoded
      b.left = left0;
      break;
    }
    bool end_of_block = false, bad = false;
    if (k == 0) {
      if (W) w->dcd[w->blk0 + w->bi] = (int16_t)(s ? qr_extend(r, s) : 0);
      k = 1;
    } else {
      const int run = sym >> 4;
      if (s) {
        k += run;
        if (k > 63) bad = true;
        else {
          if (W && blk) blk[zz[k]] = (int16_t)qr_extend(r, s);
          end_of_block = ++k == 64;
        }
      } else if (run != 15) {
        end_of_block = true;                                       // EOB
      } else {
        if (k + 15 > 63) bad = true;
        else end_of_block = (k += 16) == 64;
      }
    }
    if (bad) {
      if (W) {
        w->status = QS_RD_CODE;
        break;
      }
      k = 0;
      continue;
    }
    if (end_of_block) {
      k = 0;
      um = um + 1 == S.period ? 0 : um + 1;
      ++done;
      if (W) {
        if (++w->bi >= w->nblk) {                                  // the interval's last block: a whole byte unread?
          if (b.pos < b.end || b.left - b.pad >= 8) w->status = QS_RD_LENGTH;
          break;
        }
        blk = qrs_block(S, *w, w->bi);
      }
    }
    p = qrs_pos(b, ff);
  }
  *exit = qrs_pack(p, k, um);
  *cnt = done;
}

// the interval of segment j and its place in it: seg0[r] <= j < seg0[r + 1]
QS_RD_HD int qrs_find_interval(const uint32_t* seg0, int intervals, uint32_t j) {
  int lo = 0, hi = intervals;
  for (int i = 0; i < 32 && hi - lo > 1; ++i) {
    const int mid = lo + (hi - lo) / 2;
    if (seg0[mid] <= j) lo = mid; else hi = mid;
  }
  return lo;
}

// bytes [*start, *stop) of interval r, from the marker kernels' P and the scan's end
QS_RD_HD void qrs_interval_bytes(const uint64_t* P, int r, uint64_t end, uint64_t* start, uint64_t* stop) {
  uint64_t a = P[r], z = P[r + 1] - 2;
  if (z > end) z = end;
  if (a > z) a = z;
  *start = a;
  *stop = z;
}

// one lane of the speculative pass (round 0) or of synchronisation launch `round` (1 ..)
QS_RD_HD void qrs_lane(const QrJob& J, const QrsJob& S, const QrTable* tab, const QrSrc& src, uint64_t end,
                       const uint64_t* P, const QrsBufs& B, uint32_t j, int round) {
  const int r = qrs_find_interval(B.seg0, J.intervals, j);
  const uint32_t s = j - B.seg0[r];
  const uint64_t* from = (round & 1) ? B.exit[0] : B.exit[1];
  uint64_t* to = (round & 1) ? B.exit[1] : B.exit[0];
  uint64_t entry;
  uint64_t start, stop;
  qrs_interval_bytes(P, r, end, &start, &stop);
  if (round == 0) {
    entry = qrs_pack(qrs_bound(src, start, stop, s) * 8, 0, 0);    // (segment 0: the interval's start, known)
  } else {
    entry = s ? from[j - 1] : B.entry[j];
    if (entry == B.entry[j]) {
      to[j] = from[j];
      return;
    }
  }
  B.entry[j] = entry;
  const uint64_t lo = qrs_bound(src, start, stop, s);
  const uint64_t hi = (s + 1 == B.seg0[r + 1] - B.seg0[r]) ? stop : qrs_bound(src, start, stop, (uint64_t)s + 1);
  uint32_t cnt;
  qrs_walk<false>(tab, S, src, stop, lo, hi, entry, &to[j], &cnt, nullptr);
  B.cnt[j] = cnt;
}

// ---- the whole job, one step after the other (host builds: tests/read_split_host.cpp) -------------------------------------
// The stages of qs_kernels_read_split.hip restated serially on the same functions.  `rounds`: synchronisation rounds
// to run (the kernels': QS_RD_SPLIT_ROUNDS).  *needed (may be null): the rounds after which every link held, -1: not
// within `rounds`.  B: arrays of qrs_max_segments() elements (seg0: intervals + 1; dcd: nblocks).
QS_RD_HD int qr_split_serial(const QrJob& J, const QrSrc& scan, const QrOut& out, const QrsBufs& B, uint64_t* P, int rounds,
                             int* needed) {
  if (needed) *needed = -1;
  for (int c = 0; c < J.g.ncomp; ++c)
    for (long long i = 0; i < (long long)out.nblk[c] * 64; ++i) out.coef[c][i] = 0;
  QrSrc s = scan;
  if (s.n > J.max_scan) s.n = J.max_scan;
  uint64_t end = s.n;
  for (uint64_t p = 0; p < s.n; ++p)
    if (qr_marker(qr_byte(s, p), qr_byte(s, p + 1)) == 2) {
      end = p;
      break;
    }
  int nmark = 0, status = QS_RD_OK;
  P[0] = 0;
  for (uint64_t p = 0; p < end; ++p)
    if (qr_marker(qr_byte(s, p), qr_byte(s, p + 1)) == 1) {
      if (qr_byte(s, p + 1) != 0xD0u + (uint32_t)(nmark & 7)) status = QS_RD_MARKERS;
      ++nmark;
      if (nmark < J.intervals) P[nmark] = p + 2;
    }
  P[J.intervals] = end + 2;
  if (nmark != J.intervals - 1) status = QS_RD_MARKERS;
  if (status) return status;
  QrSrc body = s;
  body.n = end;
  QrsJob S;
  memset(&S, 0, sizeof S);
  qrs_describe(J, &S);
  // the segment map
  uint32_t nseg = 0;
  for (int r = 0; r < J.intervals; ++r) {
    uint64_t a, z;
    qrs_interval_bytes(P, r, end, &a, &z);
    B.seg0[r] = nseg;
    nseg += (uint32_t)qrs_segments(a, z);
  }
  B.seg0[J.intervals] = nseg;
  *B.nseg = nseg;
  // the speculative pass and the synchronisation rounds; every round reads what the round before left
  for (int round = 0; round <= rounds; ++round) {
    for (uint32_t j = 0; j < nseg; ++j) qrs_lane(J, S, J.tab, body, end, P, B, j, round);
    if (needed && *needed < 0) {
      bool ok = true;
      for (int r = 0; r < J.intervals && ok; ++r)
        for (uint32_t j = B.seg0[r] + 1; j < B.seg0[r + 1] && ok; ++j)
          ok = B.entry[j] == ((round & 1) ? B.exit[1] : B.exit[0])[j - 1];
      if (ok) *needed = round;
    }
  }
  // verify and count
  const uint64_t* last = (rounds & 1) ? B.exit[1] : B.exit[0];
  for (int r = 0; r < J.intervals; ++r)
    for (uint32_t j = B.seg0[r] + 1; j < B.seg0[r + 1]; ++j)
      if (B.entry[j] != last[j - 1]) return QS_RD_NOSYNC;
  // the write pass
  for (int r = 0; r < J.intervals; ++r) {
    const int m0 = r * J.ri, m1 = (m0 + J.ri < J.g.mcus) ? m0 + J.ri : J.g.mcus;
    uint64_t a, z;
    qrs_interval_bytes(P, r, end, &a, &z);
    long long first = 0;
    for (uint32_t j = B.seg0[r]; j < B.seg0[r + 1]; ++j) {
      const uint32_t sg = j - B.seg0[r];
      QrsSink w;
      w.g = &J.g;
      w.out = out;
      w.dcd = B.dcd;
      w.blk0 = (long long)m0 * J.g.bpm;
      w.nblk = (long long)(m1 - m0) * J.g.bpm;
      w.bi = first;
      w.status = QS_RD_OK;
      const uint64_t lo = qrs_bound(body, a, z, sg);
      const uint64_t hi = j + 1 == B.seg0[r + 1] ? z : qrs_bound(body, a, z, (uint64_t)sg + 1);
      uint64_t ex;
      uint32_t cnt;
      qrs_walk<true>(J.tab, S, body, z, lo, hi, B.entry[j], &ex, &cnt, &w);
      if (w.status > status) status = w.status;
      first += B.cnt[j];
    }
    if (first < (long long)(m1 - m0) * J.g.bpm && status < QS_RD_LENGTH) status = QS_RD_LENGTH;
  }
  if (status) return status;
  // the DC pass: the prediction restarts with every interval and is carried as libjpeg's int, stored as JCOEF
  QrsSink w;
  w.g = &J.g;
  w.out = out;
  w.blk0 = 0;
  uint32_t pred[4] = {0, 0, 0, 0};
  for (int m = 0; m < J.g.mcus; ++m) {
    if (m % J.ri == 0) pred[0] = pred[1] = pred[2] = pred[3] = 0;
    for (int u = 0; u < J.g.bpm; ++u) {
      const long long gi = (long long)m * J.g.bpm + u;
      pred[S.comp[u] & 3] += (uint32_t)(int32_t)B.dcd[gi];
      int16_t* blk = qrs_block(S, w, gi);
      if (blk) blk[0] = (int16_t)pred[S.comp[u] & 3];
    }
  }
  return QS_RD_OK;
}

// ---- what a run passes to the split kernels ----------------------------------------------------------------------------------
struct QrsArgs {
  QrArgs a;                        // as the init and marker kernels take it
  const QrsJob* sjobs;             // the chunk's split descriptors (workspace)
  int32_t swg0[QS_RD_CHUNK];       // each job's first workgroup in the launches over segments ...
  int32_t twg0[QS_RD_CHUNK];       // ... and in those over MCUs
  int32_t round, pad;
};
