/*
 * geom_host.cpp -- the scan reader's geometry (csrc/qs_read.h: qr_geometry) on the host, for tests/test_scan_geometry.py:
 * one line per case of the grid
 *
 *   ncomp 1 and 3  x  W, H in {1, 7, 8, 9, 16, 17, 65500}  x  luma h, v in 1..4 (chroma 1x1)
 *
 * with arrays large enough for every case:  ncomp W H h v  rc bpm mcus  nw[0] nh[0] nw[1] nh[1] nw[2] nh[2]
 */
#include <stdint.h>
#include <stdio.h>

#include "qs_read.h"

int main() {
  const int sizes[7] = {1, 7, 8, 9, 16, 17, 65500};
  const int32_t big[4] = {1 << 15, 1 << 15, 1 << 15, 1 << 15};
  for (int ncomp = 1; ncomp <= 3; ncomp += 2)
    for (int W : sizes)
      for (int H : sizes)
        for (int h = 1; h <= 4; ++h)
          for (int v = 1; v <= 4; ++v) {
            const int32_t hs[4] = {h, 1, 1, 0}, vs[4] = {v, 1, 1, 0};
            QsEncGeom g;
            const int rc = qr_geometry(ncomp, W, H, hs, vs, big, big, &g);
            printf("%d %d %d %d %d  %d %d %d ", ncomp, W, H, h, v, rc, g.bpm, g.mcus);
            for (int c = 0; c < 3; ++c) printf(" %d %d", g.nw[c], g.nh[c]);
            printf("\n");
          }
  return 0;
}
