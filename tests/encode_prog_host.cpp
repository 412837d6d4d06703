// encode_prog_host.cpp -- csrc/qs_encode_prog.h on the host: the script validation, the per-scan geometry, the block
// coders and the serial restatement of a scan, with the optimal tables of csrc/qs_huff.h, as a program of its own
// (tests/test_encode_prog_host.py builds it plain and with -fsanitize=address,undefined).
//   encode_prog_host write IN SCRIPT HEAD OUT restart_interval restart_in_rows
//   encode_prog_host validate NCOMP SCRIPT      -> prints the QP_SCRIPT_* code and the scan
//   encode_prog_host bounds                     -> checks the per-block bounds of the header by construction
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

// the worst block of each kind really takes the bits the header states
static int bounds() {
  struct Count {
    uint32_t bits = 0;
    void dc(int, int cat, uint32_t) { bits += 16 + cat; }
    void ac(int, int, uint32_t, int nb) { bits += 16 + nb; }
  };
  int bad = 0;
  for (int Ss = 1; Ss <= 63; ++Ss)
    for (int Se = Ss; Se <= 63; ++Se) {
      int16_t v[64];
      for (int i = 0; i < 64; ++i) v[i] = 1023;
      Count c;
      qp_ac_first(v, Ss, Se, 0, 0, c);
      qp_eobrun(QP_EOB_MAX, 0, c);
      if (c.bits != (uint32_t)QP_AC_MAXBITS(Ss, Se) || c.bits > QP_MAXBITS) ++bad;
    }
  Count d;
  qp_dc_first(2047, 0, d);
  if (d.bits != QP_DC_MAXBITS) ++bad;
  if (QP_MAXBITS > 0xffff || QP_LDS_WORDS * 4 > 60 * 1024) ++bad;
  printf("bounds %s: AC 1..63 %d bits, DC %d bits, %d LDS words\n", bad ? "BAD" : "ok", QP_MAXBITS, QP_DC_MAXBITS, QP_LDS_WORDS);
  return bad ? 1 : 0;
}

int main(int argc, char** argv) {
  if (argc == 2 && !strcmp(argv[1], "bounds")) return bounds();
  if (argc == 4 && !strcmp(argv[1], "validate")) {
    const std::vector<QpScanRec> s = read_script(argv[3]);
    int scan = -1;
    const char* why = "";
    // exactly the script's records on the heap: a read past them is a sanitizer report
    std::unique_ptr<QpScanRec[]> recs(new QpScanRec[s.size() ? s.size() : 1]);
    for (size_t i = 0; i < s.size(); ++i) recs[i] = s[i];
    const int code = qp_validate_script(recs.get(), (int)s.size(), atoi(argv[2]), &scan, &why);
    printf("%d %d %s\n", code, scan, why);
    return 0;
  }
  if (argc != 8 || strcmp(argv[1], "write")) {
    fprintf(stderr, "usage: encode_prog_host write IN SCRIPT HEAD OUT restart_interval restart_in_rows\n");
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
  if (qp_validate_script(script.data(), (int)script.size(), n, &scan, &why) != QP_SCRIPT_OK) {
    fprintf(stderr, "encode_prog_host: scan %d: %s\n", scan, why);
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
    const QpScanRec& r = script[si];
    QsEncGeom gs;
    if (qp_scan_geometry(full, r, &gs, &detail) != QS_GEOM_OK) {
      fprintf(stderr, "encode_prog_host: scan %zu: %d blocks in an MCU\n", si, detail);
      return 5;
    }
    int32_t tbl[4] = {0, 0, 0, 0};
    for (int c = 0; c < r.ncomp; ++c) tbl[c] = tblf[r.comp[c]];
    const long ri = rows_arg > 0 ? (rows_arg * (long)gs.mcus_x < 65535 ? rows_arg * (long)gs.mcus_x : 65535) : ri_arg;
    // the histogram, the optimal tables of this scan, their code words
    static uint32_t hist[4][257];
    memset(hist, 0, sizeof hist);
    QpHistSink hsink{hist};
    uint32_t flags = qp_scan_serial(gs, A, r, tbl, (int)ri, hsink, [](int) {});
    if (flags & QS_ENC_F_BADCOEF) status = status > 1 ? status : 1;
    uint32_t dcw[2][16], acw[2][256];
    memset(dcw, 0, sizeof dcw);
    memset(acw, 0, sizeof acw);
    bool sent[4] = {false, false, false, false};
    for (int c = 0; c < r.ncomp; ++c) {
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
      out.push_back((uint8_t)(r.Ss == 0 ? tbl[c] << 4 : tbl[c]));
    }
    out.push_back((uint8_t)r.Ss);
    out.push_back((uint8_t)r.Se);
    out.push_back((uint8_t)((r.Ah << 4) | r.Al));
    // the segment, into a buffer sized by the header's bound: every byte stuffed, a pad byte and a marker per interval
    const uint64_t mb = r.Ss == 0 ? QP_DC_MAXBITS : QP_AC_MAXBITS(r.Ss, r.Se);
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
    if (bytes.n > cap) {
      fprintf(stderr, "encode_prog_host: scan %zu: %llu bytes pass the bound of %llu\n", si, (unsigned long long)bytes.n,
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
