/*
 * encode_plan_host.cpp -- the part of csrc/qs_encode_plan.h that needs no HIP, on the host, for
 * tests/test_encode_plan_host.py: the registry of prepared workspaces (QsPrepared) and the restart rule (qs_enc_restart).
 * Prints one line per failed check and returns their number.
 */
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "qs_encode_plan.h"

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { printf("line %d: %s\n", __LINE__, #cond); ++failures; } } while (0)

static void registry() {
  QsPrepared<std::vector<int>> reg(3);
  const void *A = (const void*)0x100, *B = (const void*)0x200, *C = (const void*)0x300, *D = (const void*)0x400,
             *E = (const void*)0x500;
  CHECK(!reg.find(A));                                      // unknown
  reg.store(A, {1});
  reg.store(B, {2});
  reg.store(C, {3});
  CHECK(reg.find(A) && reg.find(B) && reg.find(C));         // three entries: the cap holds them
  CHECK((*reg.find(B))[0] == 2);
  reg.store(D, {4});                                        // the fourth store: A, stored longest ago, goes
  CHECK(!reg.find(A));
  CHECK(reg.find(B) && reg.find(C) && reg.find(D));
  reg.store(B, {20});                                       // B again: its age is refreshed, a lookup does not refresh one
  CHECK(reg.find(C));
  reg.store(E, {5});                                        // so C is the oldest now
  CHECK(!reg.find(C));
  CHECK(reg.find(B) && (*reg.find(B))[0] == 20);
  CHECK(reg.find(D) && reg.find(E));
  // what a lookup handed out stays valid when the address is stored again, and when the entry is evicted
  std::shared_ptr<const std::vector<int>> held = reg.find(B);
  reg.store(B, {21, 22});
  CHECK(held && held->size() == 1 && (*held)[0] == 20);
  CHECK(reg.find(B)->size() == 2 && (*reg.find(B))[1] == 22);
  std::shared_ptr<const std::vector<int>> old = reg.find(D);
  reg.store(A, {1});                                        // D (stored before E and B) goes
  CHECK(!reg.find(D));
  CHECK(old && (*old)[0] == 4);
  // two registries do not see each other's entries (one per route)
  QsPrepared<int> other(3);
  other.store(A, 7);
  CHECK(*other.find(A) == 7 && (*reg.find(A))[0] == 1);
  CHECK(!other.find(B));
}

static void restart_rule() {
  // the scans of the grid of tests/test_encode_plan_record.py: MCUs per row, MCUs; restart_interval, restart_in_rows
  // -> the kernels' interval, the DRI value
  static const struct { int mcus_x, mcus, interval, rows, want, dri; } T[] = {
      {1, 1, 0, 0, 0, 0},             {1, 1, 1, 0, 0, 1},           {1, 1, 0, 1, 0, 1},        {1, 1, 0, 9, 0, 9},            // gray 8 x 8
      {257, 257, 0, 0, 0, 0},         {257, 257, 1, 0, 1, 1},       {257, 257, 256, 0, 256, 256},                             // gray 2056 x 8
      {257, 257, 257, 0, 0, 257},     {257, 257, 0, 1, 0, 257},     {257, 257, 0, 9, 0, 2313},
      {2, 4, 0, 0, 0, 0},             {2, 4, 1, 0, 1, 1},           {2, 4, 3, 0, 3, 3},        {2, 4, 4, 0, 0, 4},            // YCbCr 2x2, 32 x 32
      {2, 4, 0, 1, 2, 2},             {2, 4, 5, 1, 2, 2},           {2, 4, 0, 9, 0, 18},
      {4, 16, 0, 1, 4, 4},            {4, 16, 0, 3, 12, 12},        {4, 16, 16, 0, 0, 16},     {4, 16, 0, 9, 0, 36},          // its 1x1 variant
      {4, 8, 0, 1, 4, 4},             {4, 8, 0, 2, 0, 8},           {4, 8, 7, 0, 7, 7},                                       // CMYK, component 0 alone
      {8188, 81880, 1, 0, 1, 1},      {8188, 81880, 0, 1, 8188, 8188},   {8188, 81880, 0, 8, 65504, 65504},                   // gray 65500 x 80
      {8188, 81880, 0, 9, 65535, 65535},   {8188, 81880, 65535, 0, 65535, 65535},   {8188, 81880, 0, 2147483647, 65535, 65535},
  };
  for (const auto& t : T) {
    QsEncGeom g = QsEncGeom();
    g.mcus_x = t.mcus_x;
    g.mcus = t.mcus;
    int dri = -1;
    const int got = qs_enc_restart(t.interval, t.rows, g, &dri);
    if (got != t.want || dri != t.dri || qs_enc_restart(t.interval, t.rows, g) != t.want) {
      printf("restart rule: %d x %d MCUs, interval %d, rows %d: %d / DRI %d, want %d / %d\n", t.mcus_x, t.mcus / t.mcus_x,
             t.interval, t.rows, got, dri, t.want, t.dri);
      ++failures;
    }
  }
}

int main() {
  registry();
  restart_rule();
  if (!failures) printf("ok\n");
  return failures;
}
