// huff_host.cpp -- csrc/qs_huff.h on the host: the table procedure of the device's table kernel in its host form, as a
// program of its own (tests/test_huff_host.py builds it plain and with -fsanitize=address,undefined).
//   huff_host run IN OUT
// IN:  int32 n, then n histograms of 256 uint32 counts.
// OUT: per histogram int32 status (0, or 5 for a code length above 32), bits[17], huffval[256].
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <memory>
#include <vector>

#include "qs_huff.h"

int main(int argc, char** argv) {
  if (argc != 4 || strcmp(argv[1], "run")) {
    fprintf(stderr, "usage: huff_host run IN OUT\n");
    return 2;
  }
  FILE* f = fopen(argv[2], "rb");
  if (!f) return 3;
  int32_t n = 0;
  if (fread(&n, 4, 1, f) != 1 || n < 0 || n > (1 << 20)) return 3;
  // exactly 256 counts per histogram on the heap: a read of counts[256] or counts[-1] is a sanitizer report
  std::vector<std::unique_ptr<uint32_t[]>> hist;
  for (int i = 0; i < n; ++i) {
    hist.emplace_back(new uint32_t[256]);
    if (fread(hist.back().get(), 4, 256, f) != 256) return 3;
  }
  fclose(f);
  FILE* o = fopen(argv[3], "wb");
  if (!o) return 3;
  for (int i = 0; i < n; ++i) {
    std::unique_ptr<QsHuffShared> S(new QsHuffShared);
    memset(S.get(), 0xA5, sizeof(QsHuffShared));                  // nothing may depend on what the memory held
    const int32_t status = qs_huff_wave(hist[(size_t)i].get(), *S);
    fwrite(&status, 4, 1, o);
    fwrite(S->outbits, 1, 17, o);
    fwrite(S->huffval, 1, 256, o);
  }
  fclose(o);
  return 0;
}
