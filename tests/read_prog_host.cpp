/*
 * read_prog_host.cpp -- the progressive route of the device scan reader (csrc/qs_read_prog.h) compiled for the host, for
 * tests/test_read_prog_host.py: the same block decoders, interval decode, geometry and level assignment a GPU lane and
 * its driver run, on cases read from a file.  Also built with -fsanitize=address,undefined and run on a corrupt corpus:
 * every file lies in a heap block of exactly its size, at a varying offset from 16-byte alignment, and every array
 * between guard margins that are checked after the run.
 *
 *   read_prog_host run in.bin out.bin
 *   read_prog_host correct p1 coef byte [p1 coef byte ...]
 *
 * correct: qrp_correct on one coefficient with the one-byte stream `byte`, per triple a line "coef bits": the coefficient
 * behind the call and the bits the call took.  No file validate_script accepts hands the function a coefficient whose bit
 * Al is set, so its guard is pinned here, at block level.
 *
 * in.bin:  int32 ncases, then per case
 *            int32 ncomp, width, height, hsamp[4], vsamp[4], stride[4] (blocks per array row), rows[4], nscans
 *            per scan: int32 ns, comp[4], Ss, Se, Ah, Al, Td[4], Ta[4], DRI; uint64 offset;
 *                      8 tables (DC 0..3, AC 0..3): uint8 present, bits[17], huffval[256]
 *            uint64 file_bytes, the file
 * out.bin: per case int32 status -- 0..3 as d_status, -1 a used table that is no Huffman table, -2 geometry refused, -3
 *          over the interval cap, -4 more than 10 blocks in an MCU, -5 the script is refused, -6 a store outside an
 *          array -- int32 levels and, for status >= 0, the arrays (stride x rows x 64 int16 per component)
 */
#include "qs_read_prog.h"
#include "read_case.h"                    // get, rc_table

static const int GUARD = 256;      // int16 on either side of every array

static int run(const char* src, const char* dst) {
  FILE *in = fopen(src, "rb"), *out = fopen(dst, "wb");
  int32_t ncases = 0;
  if (!in || !out || !get(in, &ncases, 4) || ncases < 0) {
    fprintf(stderr, "read_prog_host: bad input\n");
    return 1;
  }
  for (int ci = 0; ci < ncases; ++ci) {
    int32_t h[3 + 4 * 4 + 1];
    if (!get(in, h, sizeof h)) return 1;
    const int32_t *hs = h + 3, *vs = h + 7, *stride = h + 11, *rows = h + 15;
    const int ncomp = h[0], nscans = h[19];
    if (nscans < 0 || nscans > 4096) return 1;
    int32_t status = 0, levels = 0;
    std::vector<QrJob> J((size_t)nscans);
    std::vector<QrpScan> X((size_t)nscans);
    std::vector<QpScanRec> recs((size_t)nscans);
    std::vector<int32_t> level((size_t)nscans);
    QsEncGeom full;
    int detail = 0;
    if (qrp_frame_geometry(ncomp, h[1], h[2], hs, vs, stride, rows, &full, &detail) != QS_GEOM_OK) status = -2;
    for (int s = 0; s < nscans; ++s) {
      int32_t r[18];
      uint64_t offset = 0;
      if (!get(in, r, sizeof r) || !get(in, &offset, 8)) return 1;
      memset(&J[(size_t)s], 0, sizeof(QrJob));
      memset(&X[(size_t)s], 0, sizeof(QrpScan));
      memcpy(&recs[(size_t)s], r, sizeof(QpScanRec));
      uint8_t tabs[8][RC_TABLE_REC];
      if (!get(in, tabs, sizeof tabs)) return 1;
      if (status) continue;
      const QpScanRec& rec = recs[(size_t)s];
      if (rec.ncomp < 1 || rec.ncomp > 4) {
        status = -5;
        continue;
      }
      bool bad = false;
      for (int c = 0; c < rec.ncomp; ++c) bad |= rec.comp[c] < 0 || rec.comp[c] >= ncomp;
      if (bad) {
        status = -5;
        continue;
      }
      long long d = 0;
      const int why = qrp_describe(full, rec, r + 9, r + 13, r[17], offset, 0, &J[(size_t)s], &X[(size_t)s], &d);
      if (why) {
        status = why == QRP_MCU ? -4 : why == QRP_CAP ? -3 : -1;
        continue;
      }
      for (int c = 0; c < rec.ncomp; ++c) {
        const int t = rec.Ss == 0 ? J[(size_t)s].dc_tbl[c] : 4 + J[(size_t)s].ac_tbl[c];
        if (rec.Ss == 0 && rec.Ah) continue;                           // a DC refinement has no symbols
        if (!tabs[t][0] || rc_table(tabs[t], t, &J[(size_t)s].tab[t])) status = -1;
      }
    }
    uint64_t n = 0;
    if (!get(in, &n, 8) || n > (1u << 30)) return 1;
    // exactly n bytes, `shift` bytes behind a 16-byte boundary
    const size_t shift = (size_t)ci % 16;
    uint8_t* heap = static_cast<uint8_t*>(malloc(shift + n ? shift + n : 1));   // (malloc aligns to 16 bytes)
    if (!heap) return 1;
    uint8_t* file = heap + shift;
    if (n && !get(in, file, (size_t)n)) return 1;
    if (status == 0) {
      int bad = -1;
      const char* why = "";
      const int v = qp_validate_script(recs.data(), nscans, ncomp, &bad, &why);
      if ((v != QP_SCRIPT_OK && v != QP_SCRIPT_REFINE) || nscans > QRP_MAX_SCANS) status = -5;
    }
    if (status == 0) {
      levels = qrp_levels(recs.data(), nscans, level.data());
      for (int s = 0; s < nscans; ++s) {
        X[(size_t)s].level = level[(size_t)s];
        if (s + 1 < nscans) X[(size_t)s].limit = X[(size_t)s + 1].offset;
      }
      std::vector<std::vector<int16_t>> arr((size_t)ncomp);
      QrOut o;
      memset(&o, 0, sizeof o);
      for (int c = 0; c < ncomp; ++c) {
        arr[(size_t)c].assign((size_t)stride[c] * rows[c] * 64 + 2 * GUARD, (int16_t)0x5a5a);
        o.coef[c] = arr[(size_t)c].data() + GUARD;
        o.nblk[c] = stride[c] * rows[c];
      }
      QrSrc s;
      s.p = file;
      s.n = n;
      status = qrp_read_serial(J.data(), X.data(), nscans, ncomp, s, o);
      for (int c = 0; c < ncomp; ++c)
        for (int i = 0; i < GUARD; ++i)
          if (arr[(size_t)c][(size_t)i] != (int16_t)0x5a5a || arr[(size_t)c][arr[(size_t)c].size() - 1 - (size_t)i] != (int16_t)0x5a5a)
            status = -6;
      fwrite(&status, 4, 1, out);
      fwrite(&levels, 4, 1, out);
      if (status >= 0)
        for (int c = 0; c < ncomp; ++c) fwrite(arr[(size_t)c].data() + GUARD, 2, arr[(size_t)c].size() - 2 * GUARD, out);
    } else {
      fwrite(&status, 4, 1, out);
      fwrite(&levels, 4, 1, out);
    }
    free(heap);
  }
  fclose(in);
  return fclose(out) != 0;
}

static int correct(int n, char** v) {
  for (int i = 0; i + 2 < n; i += 3) {
    const uint8_t byte = (uint8_t)atoi(v[i + 2]);
    int16_t c = (int16_t)atoi(v[i + 1]);
    QrSrc s;
    s.p = &byte;
    s.n = 1;
    QrBits b;
    qr_bits_init(b, s, 0, 1);
    qr_fill(b);
    const int before = b.left;
    qrp_correct(b, atoi(v[i]), &c);
    printf("%d %d\n", (int)c, before - b.left);
  }
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 4 && !strcmp(argv[1], "run")) return run(argv[2], argv[3]);
  if (argc >= 5 && (argc - 2) % 3 == 0 && !strcmp(argv[1], "correct")) return correct(argc - 2, argv + 2);
  fprintf(stderr, "usage: read_prog_host run in.bin out.bin | correct p1 coef byte ...\n");
  return 2;
}
