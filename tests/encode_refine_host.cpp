// encode_refine_host.cpp -- csrc/qs_encode_prog.h on the host for scripts with refinement scans (Ah > 0): the block
// coders qr_dc_refine / qr_ac_refine and the serial restatement qp_scan_serial in libjpeg's order of events, with the
// optimal tables of csrc/qs_huff.h, as a program of its own (tests/test_encode_refine_host.py builds it plain and with
// -fsanitize=address,undefined).  tests/encode_prog_host.cpp for every script libjpeg takes as progressive.
//   encode_refine_host write IN SCRIPT HEAD OUT restart_interval restart_in_rows
//   encode_refine_host bounds      -> checks the per-block bounds of the refinement coders by construction
// IN: the arrays in the format of tests/libjpeg9_decode.c.  SCRIPT: one scan per line, "ncomp c0 c1 c2 c3 Ss Se Ah Al".
// HEAD: SOI .. SOF2.  OUT: the file.  Exit status 0 written, 4 a refused coefficient or table (status on stdout), 5 a scan
// with more than 10 blocks in an MCU, 3 bad input.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <memory>
#include <vector>

#include "qs_encode_prog.h"
#include "qs_huff.h"

#define MAGIC 0x51534a43

static std::vector<uint8_t> slurp(const char* path) {
  std::vector<uint8_t> v;
  FILE* f = fopen(path, "rb");
  if (!f) exit(3);
  uint8_t buf[65536];
  size_t n;
  while ((n = fread(buf, 1, sizeof buf, f)) > 0) v.insert(v.end(), buf, buf + n);
  fclose(f);
  return v;
}

static std::vector<QpScanRec> read_script(const char* path) {
  std::vector<QpScanRec> s;
  FILE* f = fopen(path, "r");
  if (!f) exit(3);
  QpScanRec r;
  while (fscanf(f, "%d %d %d %d %d %d %d %d %d", &r.ncomp, &r.comp[0], &r.comp[1], &r.comp[2], &r.comp[3], &r.Ss, &r.Se, &r.Ah,
                &r.Al) == 9)
    s.push_back(r);
  fclose(f);
  return s;
}

struct Count {
  uint32_t bits = 0;
  void ac(int, int, uint32_t, int nb) { bits += 16 + nb; }
  void raw(uint32_t, int nb) { bits += nb; }
};

// The worst block of a refinement scan really takes the bits the header states: every band coefficient newly nonzero
// but the last, which leaves one correction bit in the buffer so that the block can start a run piece, of the longest
// run.  No block of a pseudo-random sample over {0, +-1, +-2, +-3} takes more, with or without a piece.
static int bounds() {
  int bad = 0;
  uint32_t lcg = 12345;
  for (int Ss = 1; Ss <= 63; ++Ss)
    for (int Se = Ss; Se <= 63; ++Se) {
      int16_t v[64];
      for (int i = 0; i < 64; ++i) v[i] = (i & 1) ? 1 : -1;
      v[QP_ZZ[Se]] = 2;
      Count c;
      const uint32_t f = qr_ac_block(v, Ss, Se, 0, 0, QP_EOB_MAX, c);
      if (c.bits != (uint32_t)QR_AC_MAXBITS(Ss, Se) || c.bits > QP_MAXBITS || !(f & QP_F_ENDZ)) ++bad;
      for (int rep = 0; rep < 8; ++rep) {
        for (int i = 0; i < 64; ++i) {
          lcg = lcg * 1664525u + 1013904223u;
          v[i] = (int16_t)((int)((lcg >> 24) % 7) - 3);
        }
        Count r;
        QrNullSink none;
        QrBits tail;
        const uint32_t fr = qr_ac_refine(v, Ss, Se, 0, 0, none, &tail);
        qr_ac_block(v, Ss, Se, 0, 0, (fr & QP_F_ENDZ) ? QP_EOB_MAX : 0, r);
        if (r.bits > (uint32_t)QR_AC_MAXBITS(Ss, Se) || tail.n > QR_TAIL_MAX) ++bad;
      }
    }
  Count d;
  qr_dc_refine(-3, 1, d);
  if (d.bits != QR_DC_MAXBITS) ++bad;
  if (QR_PIECE_MIN != 15 || QR_PIECE_MIN * QR_TAIL_MAX <= QR_CORR_MAX || (QR_PIECE_MIN - 1) * QR_TAIL_MAX > QR_CORR_MAX) ++bad;
  printf("bounds %s: AC refinement 1..63 %d bits, DC refinement %d bit, a piece has at least %d blocks\n", bad ? "BAD" : "ok",
         QR_AC_MAXBITS(1, 63), QR_DC_MAXBITS, QR_PIECE_MIN);
  return bad ? 1 : 0;
}

int main(int argc, char** argv) {
  if (argc == 2 && !strcmp(argv[1], "bounds")) return bounds();
  if (argc != 8 || strcmp(argv[1], "write")) {
    fprintf(stderr, "usage: encode_refine_host write IN SCRIPT HEAD OUT restart_interval restart_in_rows\n");
    return 2;
  }
  const std::vector<uint8_t> in = slurp(argv[2]), head = slurp(argv[4]);
  const std::vector<QpScanRec> script = read_script(argv[3]);
  const int ri_arg = atoi(argv[6]), rows_arg = atoi(argv[7]);
  if (in.size() < 20) return 3;
  int32_t hdr[5];
  memcpy(hdr, in.data(), 20);
  const int n = hdr[1];
  if (hdr[0] != MAGIC || n < 1 || n > 4) return 3;
  size_t pos = 20;
  int32_t g[4][5], hs[4], vs[4], stride[4], rows[4];
  for (int c = 0; c < n; ++c) {
    if (pos + 20 + 128 > in.size()) return 3;
    memcpy(g[c], in.data() + pos, 20);
    pos += 20 + 128;
    stride[c] = g[c][0];
    rows[c] = g[c][1];
    hs[c] = g[c][2];
    vs[c] = g[c][3];
  }
  // each array in an allocation of its own, exactly as large as it is
  std::vector<std::unique_ptr<int16_t[]>> arrays;
  QpArrays A;
  memset(&A, 0, sizeof A);
  for (int c = 0; c < n; ++c) {
    const size_t nb = (size_t)g[c][0] * g[c][1];
    if (pos + nb * 128 > in.size()) return 3;
    arrays.emplace_back(new int16_t[nb * 64 ? nb * 64 : 1]);
    memcpy(arrays.back().get(), in.data() + pos, nb * 128);
    pos += nb * 128;
    A.coef[c] = arrays.back().get();
    A.nblk[c] = (int32_t)nb;
  }
  int scan = -1, detail = 0;
  const char* why = "";
  std::unique_ptr<QpScanRec[]> recs(new QpScanRec[script.size() ? script.size() : 1]);
  for (size_t i = 0; i < script.size(); ++i) recs[i] = script[i];
  const int verdict = qp_validate_script(recs.get(), (int)script.size(), n, &scan, &why);
  if (verdict != QP_SCRIPT_OK && verdict != QP_SCRIPT_REFINE) {
    fprintf(stderr, "encode_refine_host: scan %d: %s\n", scan, why);
    return 3;
  }
  QsEncGeom full;
  switch (qs_enc_geometry(n, hdr[2], hdr[3], hs, vs, stride, rows, nullptr, &full, &detail)) {
    case QS_GEOM_OK: break;
    case QS_GEOM_MCU: qp_complete_frame(hdr[2], hdr[3], detail, &full); break;   // judged scan by scan below
    default: return 3;
  }
  const int cs = hdr[4];
  // jpeg_set_colorspace: component ids and table slots
  int ids[4], tblf[4];
  for (int c = 0; c < 4; ++c) {
    ids[c] = cs == 2 ? "RGB "[c] : cs == 4 ? "CMYK"[c] : c + 1;
    tblf[c] = ((cs == 3 || cs == 5) && (c == 1 || c == 2)) ? 1 : 0;
  }
  std::vector<uint8_t> out(head);
  int last_dri = 0, status = 0;
  for (size_t si = 0; si < script.size(); ++si) {
    const QpScanRec& r = recs[si];
    QsEncGeom gs;
    if (qp_scan_geometry(full, r, &gs, &detail) != QS_GEOM_OK) {
      fprintf(stderr, "encode_refine_host: scan %zu: %d blocks in an MCU\n", si, detail);
      return 5;
    }
    int32_t tbl[4] = {0, 0, 0, 0};
    for (int c = 0; c < r.ncomp; ++c) tbl[c] = tblf[r.comp[c]];
    const long ri = rows_arg > 0 ? (rows_arg * (long)gs.mcus_x < 65535 ? rows_arg * (long)gs.mcus_x : 65535) : ri_arg;
    // the histogram, the optimal tables of this scan, their code words
    std::unique_ptr<uint32_t[][257]> hist(new uint32_t[4][257]);
    memset(hist.get(), 0, 4 * 257 * sizeof(uint32_t));
    QpHistSink hsink{hist.get()};
    uint32_t flags = qp_scan_serial(gs, A, r, tbl, (int)ri, hsink, [](int) {});
    if (flags & QS_ENC_F_BADCOEF) status = status > 1 ? status : 1;
    uint32_t dcw[2][16], acw[2][256];
    memset(dcw, 0, sizeof dcw);
    memset(acw, 0, sizeof acw);
    bool sent[4] = {false, false, false, false};
    const bool tables = !(r.Ss == 0 && r.Ah);        // a DC refinement has no symbols: libjpeg writes no DHT for it
    for (int c = 0; c < r.ncomp && tables; ++c) {
      const int w = (r.Ss == 0 ? 0 : 2) + tbl[c];
      if (sent[w]) continue;
      sent[w] = true;
      std::unique_ptr<QsHuffShared> S(new QsHuffShared);
      if (qs_huff_wave(hist[w], *S) != QS_HF_OK) {
        if (status != 1) status = 5;
        continue;
      }
      uint32_t* cw = r.Ss == 0 ? dcw[tbl[c]] : acw[tbl[c]];
      uint32_t code = 0;
      int p = 0;
      for (int l = 1; l <= 16; ++l) {
        for (int i = 0; i < S->outbits[l]; ++i, ++p, ++code) cw[S->huffval[p]] = ((uint32_t)l << 16) | code;
        code <<= 1;
      }
      const int len = 2 + 1 + 16 + S->nsym;
      const uint8_t m[5] = {0xff, 0xc4, (uint8_t)(len >> 8), (uint8_t)len, (uint8_t)(((w >> 1) << 4) | (w & 1))};
      out.insert(out.end(), m, m + 5);
      out.insert(out.end(), S->outbits + 1, S->outbits + 17);
      out.insert(out.end(), S->huffval, S->huffval + S->nsym);
    }
    if (status) continue;
    if (ri != last_dri) {
      const uint8_t m[6] = {0xff, 0xdd, 0, 4, (uint8_t)(ri >> 8), (uint8_t)ri};
      out.insert(out.end(), m, m + 6);
      last_dri = (int)ri;
    }
    out.push_back(0xff);
    out.push_back(0xda);
    out.push_back(0);
    out.push_back((uint8_t)(6 + 2 * r.ncomp));
    out.push_back((uint8_t)r.ncomp);
    for (int c = 0; c < r.ncomp; ++c) {
      out.push_back((uint8_t)ids[r.comp[c]]);
      // jcmarker.c emit_sos: a DC scan names no AC table, an AC scan no DC table, a DC refinement none
      out.push_back((uint8_t)(r.Ss == 0 ? (r.Ah ? 0 : tbl[c] << 4) : tbl[c]));
    }
    out.push_back((uint8_t)r.Ss);
    out.push_back((uint8_t)r.Se);
    out.push_back((uint8_t)((r.Ah << 4) | r.Al));
    // the segment, into a buffer sized by the header's bound: every byte stuffed, a pad byte and a marker per interval
    const uint64_t mb = r.Ah ? (r.Ss == 0 ? QR_DC_MAXBITS : QR_AC_MAXBITS(r.Ss, r.Se))
                             : (r.Ss == 0 ? QP_DC_MAXBITS : QP_AC_MAXBITS(r.Ss, r.Se));
    const uint64_t nint = (ri && ri < gs.mcus) ? (uint64_t)((gs.mcus + ri - 1) / ri) : 1;
    const uint64_t cap = 2 * (((uint64_t)gs.nblocks * mb + 7) / 8 + 1) + 4 * (nint - 1);
    std::unique_ptr<uint8_t[]> seg(new uint8_t[cap]);
    QpBytes bytes{seg.get(), cap, 0};
    QpBitSink sink{&dcw[0][0], &acw[0][0], &bytes};
    qp_scan_serial(gs, A, r, tbl, (int)ri, sink, [&](int k) {
      sink.pad();
      bytes.put(0xff);
      bytes.put(0xd0 + (k & 7));
    });
    sink.pad();
    if (sink.flags & QS_ENC_F_NOCODE) {
      fprintf(stderr, "encode_refine_host: scan %zu: a symbol without a code\n", si);
      return 1;
    }
    if (bytes.n > cap) {
      fprintf(stderr, "encode_refine_host: scan %zu: %llu bytes pass the bound of %llu\n", si, (unsigned long long)bytes.n,
              (unsigned long long)cap);
      return 1;
    }
    out.insert(out.end(), seg.get(), seg.get() + bytes.n);
  }
  if (status) {
    printf("status %d\n", status);
    return 4;
  }
  out.push_back(0xff);
  out.push_back(0xd9);
  FILE* o = fopen(argv[5], "wb");
  if (!o || fwrite(out.data(), 1, out.size(), o) != out.size()) return 3;
  fclose(o);
  return 0;
}
