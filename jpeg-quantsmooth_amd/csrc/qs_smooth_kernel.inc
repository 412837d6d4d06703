// qs_smooth_kernel.inc -- body of the recovery kernel (pass B), one 8x8 block per lane.
// Included twice by qs_kernels.hip:
//   QS_SMOOTH_KERNEL_NAME   kernel symbol
//   QS_SMOOTH_SET           1: parameters come from a QsPlaneSet (one launch over the components of a
//                              job or of many jobs); undefined: one plane, blocks [blk_begin, blk_end)
// This file is the shipped form only.  Every alternative that was built and measured on the way (compiler-
// scheduled weight loads, 4 waves per SIMD with inline edge differences, v_dot2 column pass, per-term zero-weight
// branches, the per-phase cycle timeline, ablations) lives in tools/experiments/ and is compiled only by
// tools/build_variants.sh; LABNOTES.md section 4.2 has the numbers.
template <bool DIAG>
__global__ void __launch_bounds__(64 * QS_WAVES_PER_WG, QS_SMOOTH_MIN_WAVES)
#ifdef QS_SMOOTH_SET
QS_SMOOTH_KERNEL_NAME(const QsPlaneSet set, int final_clamp) {
  // the luma walk (!DIAG) keeps 20 more dwords per lane behind its coefficient columns (QS_X_*, qs_kernels.hip): one
  // stash slot, the packed neighbour pixels and the two rebalance sums -- everything at an immediate offset from `col`
  __shared__ __attribute__((aligned(16))) uint32_t lds_all[QS_WAVES_PER_WG][32 * QS_LDS_PITCH + (DIAG ? 0 : QS_X_DWORDS * 64)];
#if QS_STASH
  __shared__ uint32_t stash_all[QS_WAVES_PER_WG][2 * 8 * 64];   // (DIAG only) pass-1 outputs of two block columns per lane, see the refresh
#endif
  // (luma walk: the wave index is made scalar, so that the wave's LDS base is no per-lane value that stays live across the walk)
  const int lane = threadIdx.x & 63, wave = DIAG ? (int)(threadIdx.x >> 6) : __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  uint32_t* lds = lds_all[wave];
  uint32_t* col = lds + lane;
  const int gw = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * QS_WAVES_PER_WG + wave));
  if (gw >= set.wave0[set.n]) return;  // wave-uniform
  const int pi = qs_set_find(set, gw);
  const QsConsts* __restrict__ cst = set.ref[pi].cst;
  int16_t* __restrict__ coef = set.ref[pi].coef;
  const uint8_t* __restrict__ plane = set.ref[pi].plane;
  const int wblk = set.ref[pi].wblk, hblk = set.ref[pi].hblk, pitch = set.ref[pi].pitch;
  const int rebalance = set.ref[pi].mode & QS_PLANE_REBALANCE;
  const int nblk = wblk * hblk;
  const int base = (gw - set.wave0[pi]) * 64;
  (void)hblk;
#else
QS_SMOOTH_KERNEL_NAME(const QsConsts* __restrict__ cst, int16_t* __restrict__ coef,
                       const uint8_t* __restrict__ plane, uint8_t* __restrict__ plane_next, int rep,
                       int wblk, int hblk, int pitch,
                       int rebalance, int final_clamp, int blk_begin, int blk_end) {
  // plane_next / rep: see the fused epilogue at the end (rep = QS_PLANE_REP_TOP | QS_PLANE_REP_BOT bits)
  // blocks [blk_begin, blk_end) of the plane (linear, row-major): the whole
  // plane, or the interior / the edge block rows of a band when the halo
  // exchange is overlapped with the interior (bands.py)
  // the luma walk (!DIAG) keeps 20 more dwords per lane behind its coefficient columns (QS_X_*, qs_kernels.hip): one
  // stash slot, the packed neighbour pixels and the two rebalance sums -- everything at an immediate offset from `col`
  __shared__ __attribute__((aligned(16))) uint32_t lds_all[QS_WAVES_PER_WG][32 * QS_LDS_PITCH + (DIAG ? 0 : QS_X_DWORDS * 64)];
#if QS_STASH
  __shared__ uint32_t stash_all[QS_WAVES_PER_WG][2 * 8 * 64];   // (DIAG only) pass-1 outputs of two block columns per lane, see the refresh
#endif
  // (luma walk: the wave index is made scalar, so that the wave's LDS base is no per-lane value that stays live across the walk)
  const int lane = threadIdx.x & 63, wave = DIAG ? (int)(threadIdx.x >> 6) : __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  uint32_t* lds = lds_all[wave];
  uint32_t* col = lds + lane;
  const int nblk = blk_end;
  const int base = blk_begin + (blockIdx.x * QS_WAVES_PER_WG + wave) * 64;
#endif
  if (base >= nblk) return;  // wave-uniform
  // Workgroups of the last, partial round (the grid modulo what the chip holds at once) start when the first
  // waves of the previous round retire and would otherwise trail behind as the only waves left on their SIMDs:
  // they keep their term streams one priority level above everybody else's (see the phase priorities below).
  // Measured on MI355X (tools/bench_sizes.py, 1024 blocks per row): -9 % at 200..320 block rows, -5 % at 512,
  // -1.7 % at 1024 (8192^2), +-0 elsewhere.
  const int tail_prio = __builtin_amdgcn_readfirstlane(
      (gridDim.x > QS_RESIDENT_WG && blockIdx.x >= (gridDim.x / QS_RESIDENT_WG) * QS_RESIDENT_WG) ? 1 : 0);
  const int nvec = min(64, nblk - base) * 8;
#ifdef QS_STAGGER   /* measurement builds only (tools/build_variants.sh "@ship -DQS_STAGGER=n"): odd wave slots start 64 n cycles late */
  { unsigned hwid; asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hwid)); if (hwid & 1u) __builtin_amdgcn_s_sleep(QS_STAGGER); }
#endif

  // ---- stage the wave's 64 blocks (8 KiB contiguous): 16 B per lane per
  // load, fully coalesced, transposed through LDS into per-lane columns.
  uint4* gsrc = reinterpret_cast<uint4*>(coef) + (size_t)base * 8;
  // (luma walk) Does the wave hold a coefficient outside [-0x2000, 0x2000) -- bits 15..13 of an int16 not all equal?  No
  // job does (its dequantised coefficients pass the +-2048 range check and move by less than a quantiser < 0x800), and
  // two shortcuts of the walk rest on it, see the coefficient update.  Collected on the packed pairs as they are staged.
  uint32_t bigacc = 0;
#define QS_BIG_ACC(V) if constexpr (!DIAG) bigacc |= ((V).x ^ ((V).x << 1)) | ((V).y ^ ((V).y << 1)) | ((V).z ^ ((V).z << 1)) | ((V).w ^ ((V).w << 1))
#ifdef QS_SMOOTH_SET
  // A plane whose dequantisation pass A deferred (QS_PLANE_QUANT, wave-uniform): the coefficients in HBM are still the
  // file's quantised ones, and the products pass A formed and range-checked -- coef * qraw, wrapped to int16 -- are
  // formed again here, each lane on the eighth of a block it moves, before they go to LDS.  From there on nothing
  // differs, and the write-back below stores dequantised results as always.  A copy of the loop of its own, so that
  // the staging of every other launch stays the code it was.
  if (set.ref[pi].mode & QS_PLANE_QUANT) {
    const int m0 = (lane & 7) * 4;
    int q[8], unused = 0;
    qs_load_qraw8(cst, lane & 7, q);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int idx = j * 64 + lane;
      uint4 v = make_uint4(0, 0, 0, 0);
      if (idx < nvec) v = gsrc[idx];
      v = qs_dequant8<false>(v, q, unused);
      QS_BIG_ACC(v);
      uint32_t* dst = lds + m0 * QS_LDS_PITCH + (j * 8 + (lane >> 3));
      dst[0] = v.x; dst[QS_LDS_PITCH] = v.y; dst[2 * QS_LDS_PITCH] = v.z; dst[3 * QS_LDS_PITCH] = v.w;
    }
  } else
#endif
  {
    const int m0 = (lane & 7) * 4;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int idx = j * 64 + lane;
      uint4 v = make_uint4(0, 0, 0, 0);
      if (idx < nvec) v = gsrc[idx];
      QS_BIG_ACC(v);
      uint32_t* dst = lds + m0 * QS_LDS_PITCH + (j * 8 + (lane >> 3));
      dst[0] = v.x; dst[QS_LDS_PITCH] = v.y; dst[2 * QS_LDS_PITCH] = v.z; dst[3 * QS_LDS_PITCH] = v.w;
    }
  }

  // ---- neighbour edge pixels from the frozen plane (reference :1396-1401),
  // kept packed (4 per VGPR): [0..1] row above, [2..3] row below,
  // [4..5] column to the left, [6..7] column to the right
  const int blk = min(base + lane, nblk - 1);
  const int by = blk / wblk, bx = blk - by * wblk;
  const uint8_t* org = plane + (size_t)(by * 8 + 1) * pitch + QS_APRON_X + bx * 8;
  uint32_t edge[8];
  {
    const uint2 t = *reinterpret_cast<const uint2*>(org - pitch);
    const uint2 b = *reinterpret_cast<const uint2*>(org + (size_t)8 * pitch);
    edge[0] = t.x; edge[1] = t.y; edge[2] = b.x; edge[3] = b.y;
    uint32_t l[8], r[8];
#pragma unroll
    for (int y = 0; y < 8; ++y) {
      l[y] = org[(ptrdiff_t)y * pitch - 1];
      r[y] = org[(ptrdiff_t)y * pitch + 8];
    }
    edge[4] = l[0] | (l[1] << 8) | (l[2] << 16) | (l[3] << 24);
    edge[5] = l[4] | (l[5] << 8) | (l[6] << 16) | (l[7] << 24);
    edge[6] = r[0] | (r[1] << 8) | (r[2] << 16) | (r[3] << 24);
    edge[7] = r[4] | (r[5] << 8) | (r[6] << 16) | (r[7] << 24);
  }
  // the lane's own dwords behind the columns (luma walk): written once here, the neighbour pixels read at each refresh
  uint32_t* const xcol = col + 32 * QS_LDS_PITCH;
  if constexpr (!DIAG) {
#pragma unroll
    for (int e = 0; e < 8; ++e) xcol[(QS_X_EDGE + e) * 64] = edge[e];
    *qs_xreb(col, lds, 0) = 0; *qs_xreb(col, lds, 1) = 0;
  }
  wave_lds_sync();

  constexpr int TS = DIAG ? 272 : 160;
  // Terms read pixel DIFFERENCES only, and pixels change only at a refresh.  The luma walk (!DIAG) therefore holds no
  // pixels at all: its 56 horizontal differences dh[y * 7 + x] = px[y][x] - px[y][x + 1], its 56 vertical ones
  // dv[y * 8 + x] = px[y][x] - px[y + 1][x] and the 32 edge differences bd[] are formed once per refresh, row by row
  // behind pass 2, and every term is the eight-instruction QS_TERM_D_ASM.  Each difference is the same single f32
  // subtraction of the same two operands as before (exact: integers scaled by 2^-12), formed once instead of once
  // per coefficient.  The DIAGONALS walk has 210 differences, which cannot fit: it keeps its pixels and hoists the
  // first NH horizontal differences, as many as its 3-waves-per-SIMD register budget leaves.
  float px[DIAG ? 64 : 1];   // (DIAG) own pixels * 2^-12
  float bd[32];   // own edge pixel minus neighbour pixel, * 2^-12 (top, bottom, left, right)
  constexpr int NH = DIAG ? QS_HOIST_DIAG : 1;
  float hd[NH];              // (DIAG) the first NH horizontal differences (rows 0.., x = 0..6), held between refreshes
  float dh[DIAG ? 1 : 56], dv[DIAG ? 1 : 56];   // (luma) all interior differences

  int kfirst = 63;
#if QS_STASH
  int stash_hi = 0;   // bit 0 / 1: column 6 / 7's final pass-1 output is in its stash slot (wave-uniform)
#endif
  uint32_t chg = 0;   // (DIAG) any coefficient of this lane's block changed since the last refresh
  uint64_t chg_any = 0;   // (luma) the same as a mask of the wave's lanes: SGPRs, the refresh ballot is its only reader
#undef QS_BIG_ACC
  const bool big_wave = !DIAG && __builtin_amdgcn_ballot_w64((bigacc & 0xC000C000u) != 0) != 0;   // (wave-uniform)
  // sum c*orig, sum orig*orig over the 63 AC coefficients (rebalance step); the luma walk keeps them in LDS (xreb)
  long long reb_m0 = 0, reb_m1 = 0;
  // (luma walk) Each anti-diagonal's share of the two sums is collected in a register first and added to the 64-bit LDS
  // sum once, behind the anti-diagonal: 14 LDS additions per sum instead of 63, and no widening per coefficient.
  // Exact: in a wave without out-of-range coefficients |v| and |orig| stay below 9216 (|c| < 0x2000 plus less than a
  // quantiser < 0x800, half of one more for orig), so a product is non-negative and below 2^27, and the at most 8
  // products of an anti-diagonal add up to less than 2^30 -- no wrap in 32 bits, while the 63-term sum can pass 2^32
  // and stays 64 bits wide.  A wave WITH such a coefficient (big_wave) ignores the walk's sums altogether.
  uint32_t reb_a0 = 0, reb_a1 = 0;
  // Scalar operands.  Everything about coefficient k comes from its 16-byte record (QsConsts::rec); the weights
  // stream through two 16-SGPR buffers (WA / WB), one 16-float chunk per pipeline step (QS_ISSUE / QS_LAND below).
  const float* tabp = cst->tab;
  const int32_t* recp = &cst->rec[0][0];
  qs_w16 WA, WB;
  qs_i4 REC;                             // record of the current coefficient
  qs_i4 RECN;                            // ... of the next one, fetched by the coefficient's last step
  asm volatile("s_load_dwordx4 %0, %2, %3\n\ts_load_dwordx16 %1, %4, %5\n\ts_waitcnt lgkmcnt(0)"
               : "=&s"(REC), "=&s"(WA) : "s"(recp), "s"(63u * 16u), "s"(tabp), "s"((uint32_t)63 * (TS * 4)) : "memory");
  RECN = REC;

  // 14 zigzag anti-diagonals; the block's own pixels are re-derived from its current coefficients at the start
  // of each (reference :313-322, 1407-1409).
  // Phase priorities: a wave runs the slow phases of the coefficient walk -- the refresh IDCT (integer
  // butterflies, a third of them half-rate multiplies) and the coefficient update (division, interval, LDS
  // read-modify-write) -- at RAISED wave priority (s_setprio) and its term streams at the base priority.  With
  // three waves per SIMD the pipe idles when two of them are in a slow phase at once and the third cannot fill it
  // alone; at raised priority a wave leaves its slow phase as fast as the hardware allows and such overlaps
  // become rare (profiles/r03l_phase_prio: +12.6 % at q3, +15 % at q4, identical results).
#pragma unroll 1
  for (int g = 0; g < 14; ++g) {
    __builtin_amdgcn_s_setprio(QS_PRIO_SLOW);
    // The reference refreshes "if stale" (quantsmooth.h:1407-1409, 1562: need_refresh |= add ^ coef1).
    // A wave skips the IDCT when NONE of its 64 blocks changed a coefficient in the last
    // anti-diagonal -- the pixels and edge differences in registers are then still exact.  Free on
    // smooth image regions; never taken on noisy content (LABNOTES.md 4.2c).
    if (g == 0 || (DIAG ? __builtin_amdgcn_ballot_w64(chg != 0) != 0 : chg_any != 0)) {
      chg = 0;
      chg_any = 0;
      uint32_t ws[64];
      // 64 sign-extending 16-bit LDS reads (ds_read_i16) instead of 16 ds_read2_b32 + 48 VALU sign extensions: the kernel
      // is bound by VALU issue slots, the LDS pipe idles (refresh 940 -> 885 VALU instructions; profiles/r05g_lds16)
      if constexpr (DIAG) lds_read_block_i16(col, ws); else lds_read_block_i16_1(col, ws);
#if QS_STASH
      // Column-restricted pass 1.  Pass 1 transforms block COLUMNS, and column x only holds coefficients of the
      // anti-diagonals 7 - x .. 14 - x: column 0 is untouched until anti-diagonal 7, column 1 until 6; column 7 is final
      // after anti-diagonal 7, column 6 after 8.  Their pass-1 outputs (8 int32 each) are parked in LDS -- two slots per
      // lane, 4 KB per wave: what the 3-workgroups-per-CU LDS budget leaves; slot 0: column 0, later 7; slot 1: column 1,
      // later 6 -- and read back instead of recomputed: 22 of the 112 column transforms of a block-iteration become
      // eight LDS reads each (the LDS pipe idles, VALU issue is the bound).  Same integers, whoever produced them.
      // Columns 0 / 1 are stored by refresh 0, which always runs; columns 7 / 6 by the first refresh that RUNS at
      // g >= 8 / g >= 9 (the wave-uniform refresh skip may sit some out): stash_hi remembers that it happened.
      {
        // The luma walk has LDS for slot 0 alone (columns 0 and 7: 12 of the 22 saved transforms) -- the other eight
        // dwords per lane hold what its resident differences pushed out of the register file (QS_X_*).
        uint32_t* stash = DIAG ? stash_all[wave] + lane : xcol + QS_X_STASH * 64;
#pragma unroll
        for (int x = 0; x < 8; ++x) {
          uint32_t c[8];
          const bool low = x <= (DIAG ? 1 : 0), high = x >= (DIAG ? 6 : 7);
          const int slot = (x == 0 || x == 7) ? 0 : 1;
          bool reuse = false, store = false;
          if (low) { reuse = g >= 1 && g <= 7 - x; store = g == 0; }
          if (high) {
            const int fin = 15 - x;                           // first refresh at which column x is final: 8 (x = 7), 9 (x = 6)
            const bool have = (stash_hi >> (x - 6)) & 1;
            reuse = g >= fin && have; store = g >= fin && !have;
          }
          if ((low || high) && reuse) {                       // (wave-uniform)
#pragma unroll
            for (int j = 0; j < 8; ++j) c[j] = stash[(slot * 8 + j) * 64];
          } else {
#pragma unroll
            for (int j = 0; j < 8; ++j) c[j] = ws[j * 8 + x];
            idct8(c, 1024u);
#pragma unroll
            for (int j = 0; j < 8; ++j) c[j] = (uint32_t)((int32_t)c[j] >> 11);
            if ((low || high) && store) {
#pragma unroll
              for (int j = 0; j < 8; ++j) stash[(slot * 8 + j) * 64] = c[j];
              if (high) stash_hi |= 1 << (x - 6);
            }
          }
#pragma unroll
          for (int j = 0; j < 8; ++j) ws[j * 8 + x] = c[j];
        }
      }
#else
      idct_pass1(ws);
#endif
      if constexpr (!DIAG) {
        // Pass 2 row by row; behind row y its 7 horizontal differences, the 8 vertical ones against row y - 1 (eight
        // floats kept for one row) and the row's edge differences.  Operand order is the reference's: px[p] - px[p + 1],
        // px[p] - px[p + 8], own pixel minus neighbour.  The neighbour pixels come from LDS where they are needed.
        float prev[8];
#pragma unroll
        for (int y = 0; y < 8; ++y) {
          uint32_t row[8]; float o[8];
#pragma unroll
          for (int j = 0; j < 8; ++j) row[j] = ws[y * 8 + j];
          idct_pass2_row_f(row, o);
#pragma unroll
          for (int x = 0; x < 7; ++x) dh[y * 7 + x] = o[x] - o[x + 1];
          if (y > 0) {
#pragma unroll
            for (int x = 0; x < 8; ++x) dv[(y - 1) * 8 + x] = prev[x] - o[x];
          }
          if (y == 0 || y == 7) {
            const uint32_t e0 = xcol[(QS_X_EDGE + (y ? 2 : 0)) * 64], e1 = xcol[(QS_X_EDGE + (y ? 3 : 1)) * 64];
#pragma unroll
            for (int x = 0; x < 8; ++x) bd[(y ? 8 : 0) + x] = o[x] - pix_from_byte(x < 4 ? e0 : e1, x & 3);
          }
          {
            const uint32_t el = xcol[(QS_X_EDGE + 4 + (y >> 2)) * 64], er = xcol[(QS_X_EDGE + 6 + (y >> 2)) * 64];
            bd[16 + y] = o[0] - pix_from_byte(el, y & 3);
            bd[24 + y] = o[7] - pix_from_byte(er, y & 3);
          }
#pragma unroll
          for (int x = 0; x < 8; ++x) prev[x] = o[x];
          // rows stay in order: interleaved by the scheduler, their butterflies' temporaries pile up on top of the
          // 144 resident values and spill
          __builtin_amdgcn_sched_barrier(0);
        }
      } else {
#pragma unroll
      for (int y = 0; y < 8; ++y) {
        uint32_t row[8]; float o[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) row[j] = ws[y * 8 + j];
        idct_pass2_row_f(row, o);
#pragma unroll
        for (int j = 0; j < 8; ++j) px[y * 8 + j] = o[j];
      }
      // the 32 edge differences only change here, not per coefficient.  The opaque copies make hipcc redo the
      // 32 byte-to-pixel conversions at every refresh instead of hoisting them out of the loop, where they
      // ended up in 124 B/lane of scratch (+130 MB written and re-read per 8192^2 launch).
#pragma unroll
      for (int e = 0; e < 8; ++e) asm volatile("" : "+v"(edge[e]));
#pragma unroll
      for (int x = 0; x < 8; ++x) {
        bd[x]      = px[x]         - pix_from_byte(edge[0 + (x >> 2)], x & 3);
        bd[8 + x]  = px[56 + x]    - pix_from_byte(edge[2 + (x >> 2)], x & 3);
        bd[16 + x] = px[x * 8]     - pix_from_byte(edge[4 + (x >> 2)], x & 3);
        bd[24 + x] = px[x * 8 + 7] - pix_from_byte(edge[6 + (x >> 2)], x & 3);
      }
#pragma unroll
      for (int t = 0; t < NH; ++t) hd[t] = px[(t / 7) * 8 + t % 7] - px[(t / 7) * 8 + t % 7 + 1];
      }   // (DIAG)
    }
    // anti-diagonal g (walking down from k = 63) holds min(g + 1, 15 - g) coefficients
    const int len = min(g + 1, 15 - g);
    const int klast = max(kfirst - len + 1, 1);
#pragma unroll 1
    for (int k = kfirst; k >= klast; --k) {
      // Keep the interior pixel differences inside the coefficient loop: otherwise the compiler hoists all
      // 112/210 of them out of the k-loop (they only change per anti-diagonal) and pays for it in VGPRs /
      // scratch spills.  (The luma walk has no pixels: its differences are resident by design.)
      if constexpr (DIAG) {
#pragma unroll
        for (int p = 0; p < 64; ++p) asm volatile("" : "+v"(px[p]));
      }
      // Everything about coefficient k that is a function of k alone comes ready-made in the record's fourth dword
      // (QsConsts::rec, qs_tables.cpp): which sections run and in which zero-skipping form, where the coefficient lives
      // in this lane's LDS column, whether the next coefficient's first chunk is its border chunk.  Round 4 computed
      // all of that per coefficient from the natural index (~30 scalar instructions of a wave's ~95 per coefficient --
      // each an issue slot of its own when a SIMD holds one or two waves, profiles/r04a_ubench/pmc_sizes.txt).
      const int md = REC[3];
      const int x2k = (REC[0] >> 16) & 31, qk = REC[1] & 0xffff, x1k = REC[1] >> 16;
      const uint32_t lds_off = ((uint32_t)md >> QS_REC_LDS_SHIFT) & 0x3fffu;          // byte offset of coefficient i in the lane's column
      // Toolchain hazard (ROCm 7.2, gfx950): a bit_cast of element n > 0 of an inline-asm-defined
      // SGPR tuple, used directly as a VALU source operand, is emitted as element 0 (the sub-register
      // index is lost when the scalar is folded into the VOP3 operand; SALU uses are fine).  The
      // opaque copy forces a real s_mov from the right sub-register.  Caught by every parity test.
      int rs_bits = REC[2];
      asm volatile("" : "+s"(rs_bits));
      const float Rs = __builtin_bit_cast(float, rs_bits);   // 2q * 2^-12
      const uint32_t kb = (uint32_t)k * (TS * 4);
      // the NEXT coefficient's row (k - 1; for k = 1 this is row 0, which exists and whose prefetch nobody reads) ...
      const uint32_t kb_nxt = kb - (uint32_t)(TS * 4);
      const uint32_t kb_s = (uint32_t)__builtin_amdgcn_readfirstlane((int)kb);            // (SGPR operands of the chunk loads)
      const uint32_t kb_nxt_s = (uint32_t)__builtin_amdgcn_readfirstlane((int)kb_nxt);
      // ... and its first chunk: the border chunk (+256 bytes) when it has no horizontal section
      const uint32_t next_first = kb_nxt + (((uint32_t)md >> QS_REC_NXT_SHIFT) & 0x100u);
      const uint32_t after_V = DIAG ? kb + 640u : next_first;
      const uint32_t after_B = (md & QS_REC_V_ANY) ? kb + 384u : after_V;
#if QS_Q1_SKIP
      // Quantiser 1: the interval of reference :1552-1557 is the single point the coefficient already holds
      // (d0 = d1 = 0, dl = dh = a0 = coef), so whatever the 144 / 242 terms add up to, the update stores the same
      // value back and nothing is marked stale -- the whole stream is skipped (wave-uniform: a bit of the record).
      // What remains is the coefficient's share of the rebalance sums (orig = coef) and the hand-over to the next
      // coefficient: its record and first weight chunk, which the skipped last step would have fetched.
      if (__builtin_expect(md & QS_REC_Q1, 0)) {
        {   // (unconditional: without the rebalance step nobody reads the sums)
          const int c0 = *reinterpret_cast<lds_i16*>(reinterpret_cast<char*>(col) + lds_off);
          if constexpr (DIAG) {
            reb_m0 += (long long)(c0 * c0);
            reb_m1 += (long long)(c0 * c0);
          } else {
            const uint32_t sq = (uint32_t)__mul24(c0, c0);
            reb_a0 += sq;
            reb_a1 += sq;
          }
        }
        asm volatile("s_load_dwordx16 %0, %2, %3\n\ts_load_dwordx4 %1, %4, %5\n\ts_waitcnt lgkmcnt(0)"
                     : "=&s"(WA), "=&s"(RECN)
                     : "s"(tabp), "s"((uint32_t)__builtin_amdgcn_readfirstlane((int)next_first)), "s"(recp),
                       "s"((uint32_t)(k - 1) * 16u) : "memory");
        REC = RECN;
      } else
#endif
      {
      float num = 0.0f, den = 0.0f;
      // term streams at the base priority; the workgroups of a launch's last, partial round one level above (wave-uniform)
      asm volatile("s_setprio %c1\n\ts_cmp_eq_u32 %0, 0\n\ts_cbranch_scc1 1f\n\ts_setprio %c2\n1:"
                   : : "s"(tail_prio), "i"(QS_PRIO_TERMS), "i"(QS_PRIO_TERMS + 1) : "scc");
      // Structural zeros: for horizontal frequency u = i & 7 the weight T[p] - T[p+1] vanishes exactly whenever
      // (x + 1) * u is a multiple of 8 (the two cosines coincide): x = 1,3,5 for u = 4 and x = 3 for u = 2,4,6;
      // same for the vertical differences with v = i >> 3 (whole rows y).  A zero weight makes y = 0, so the term
      // adds +0 to both sums -- skipping it is exact (the host verifies the table entries are 0.0f,
      // qs_hip_consts_build).  That is 7.7 % of all terms at q3.  Decided once per SECTION: three specialised
      // copies (MODE 2: frequency 4, MODE 1: frequency 2 or 6, MODE 0: no zeros) behind one wave-uniform branch,
      // the choice being a bit of the record.

#define QS_ROW_D(W, Y) { \
        _Pragma("unroll") for (int x = 0; x < 7; ++x) { \
          QS_TERM(px[(Y) * 8 + x], px[(Y) * 8 + x + 9], W[x]) \
          QS_TERM(px[(Y) * 8 + x + 1], px[(Y) * 8 + x + 8], W[8 + x]) } }
#define QS_EDGE16(W, J0) { \
        _Pragma("unroll") for (int j = 0; j < 16; ++j) { \
          if constexpr (DIAG) QS_TERM_D(bd[(J0) + j], W[j]) \
          else QS_TERM_D_ASM(bd[(J0) + j], W[j]) } }   /* (luma: opaque, two temporaries -- scheduled freely the 16 terms' products pile up) */
      // (every term of a specialised section is an opaque 9-instruction asm block: the three copies must not share
      //  subexpressions, or hipcc hoists ~100 pixel differences above the branch and spills them)
#define QS_HOISTED_TERM(T, WT) else if ((T) < NH) QS_TERM_D_ASM(hd[(T) % NH], WT)
#define QS_ROWS_H_M(W, Y0, MODE) { \
        _Pragma("unroll") for (int yy = 0; yy < 2; ++yy) \
        _Pragma("unroll") for (int x = 0; x < 7; ++x) { \
          if (((MODE) == 2 && (x & 1)) || ((MODE) == 1 && x == 3)) {} \
          else if constexpr (!DIAG) QS_TERM_D_ASM(dh[((Y0) + yy) * 7 + x], W[yy * 8 + x]) \
          QS_HOISTED_TERM(((Y0) + yy) * 7 + x, W[yy * 8 + x]) \
          else QS_TERM_ASM(px[((Y0) + yy) * 8 + x], px[((Y0) + yy) * 8 + x + 1], W[yy * 8 + x]) } }
#define QS_ROWS_V_M(W, Y0, NY, MODE) { \
        _Pragma("unroll") for (int yy = 0; yy < (NY); ++yy) \
        _Pragma("unroll") for (int x = 0; x < 8; ++x) { \
          if (((MODE) == 2 && (((Y0) + yy) & 1)) || ((MODE) == 1 && (Y0) + yy == 3)) {} \
          else if constexpr (!DIAG) QS_TERM_D_ASM(dv[((Y0) + yy) * 8 + x], W[yy * 8 + x]) \
          else QS_TERM_ASM(px[((Y0) + yy) * 8 + x], px[((Y0) + yy) * 8 + x + 8], W[yy * 8 + x]) } }

      // "Landed" pipeline: every chunk step is  ISSUE(next chunk) ; 14-16 terms on the current one ;
      // LAND(next chunk)  -- the load's latency hides behind ~140 VALU instructions, and the wait sits at the END
      // of the step, in the same basic block as the load, so no register is in flight across a branch, a join, the
      // coefficient update or the IDCT refresh.  (hipcc may place an asm output in other registers right behind
      // the statement; with a load in flight that copies stale data.  It happened with a record prefetch that was
      // consumed several statements later -- at a control-flow join, visible only while the scalar cache was
      // cold.  csrc/check_inflight.py scans the ISA for any such access between a scalar load and its wait and
      // fails the build.)  Section lengths before any chunk are even (H 4, B 2, V 4 chunks), so a section always
      // starts in WA.  The step that fetches the next coefficient's first chunk also fetches its record
      // (QS_ISSUE_R / QS_LAND_R).  The num/den operands pin a step between the accumulations around it.
      const uint32_t rec_next = (uint32_t)(k - 1) * 16u;      // (k = 1: record 0, never used)
#define QS_ISSUE(NXT, BYTEOFF) \
      asm volatile("s_load_dwordx16 %0, %3, %4" : "=&s"(NXT), "+v"(num), "+v"(den) \
                   : "s"(tabp), "s"((uint32_t)__builtin_amdgcn_readfirstlane((int)(BYTEOFF))) : "memory")
      // a chunk of the CURRENT coefficient's row: base + row offset (one SGPR per coefficient) + immediate -- gfx950's
      // scalar loads take both, so the per-chunk s_add of round 4 is gone
#define QS_ISSUE_K(NXT, IMM) \
      asm volatile("s_load_dwordx16 %0, %3, %4 offset:%c5" : "=&s"(NXT), "+v"(num), "+v"(den) \
                   : "s"(tabp), "s"(kb_s), "i"(IMM) : "memory")
#define QS_LAND(NXT) asm volatile("s_waitcnt lgkmcnt(0)" : "+s"(NXT), "+v"(num), "+v"(den) : : "memory")
#define QS_ISSUE_R(NXT, BYTEOFF) \
      asm volatile("s_load_dwordx16 %0, %4, %5\n\ts_load_dwordx4 %1, %6, %7" : "=&s"(NXT), "=&s"(RECN), "+v"(num), "+v"(den) \
                   : "s"(tabp), "s"((uint32_t)__builtin_amdgcn_readfirstlane((int)(BYTEOFF))), "s"(recp), "s"(rec_next) : "memory")
#define QS_LAND_R(NXT) asm volatile("s_waitcnt lgkmcnt(0)" : "+s"(NXT), "+s"(RECN), "+v"(num), "+v"(den) : : "memory")
      // Row touch: the first border step -- the one step every coefficient runs -- also asks for one dword of every
      // 64-byte line of the NEXT coefficient's weight row.  The 40 / 68 KB table does not fit the 16 KB scalar cache
      // and the waves of a CU pair walk it in lock step: asked for chunk by chunk, half of the chunk loads find their
      // line missing or on its way (SQC_DCACHE_MISSES + _DUPLICATE 331 of 645 per wave); asked for a coefficient
      // ahead, all together behind ONE wait, every chunk load hits (profiles/r04k_touch: -3 % per launch at 64-128
      // block rows, +-0 at full size).  Scalar loads return out of order, so the dummy destination stays an operand
      // up to the wait: nothing else can live in that register while a load may still write it.
#define QS_T4(O) "s_load_dword %1, %4, %5 offset:" #O "\n\ts_load_dword %1, %4, %5 offset:" #O "+0x40\n\ts_load_dword %1, %4, %5 offset:" #O "+0x80\n\ts_load_dword %1, %4, %5 offset:" #O "+0xc0\n\t"
#define QS_ISSUE_T(NXT, IMM) \
      uint32_t touch; \
      if (DIAG) asm volatile("s_load_dwordx16 %0, %4, %6 offset:%c7\n\t" QS_T4(0x0) QS_T4(0x100) QS_T4(0x200) QS_T4(0x300) "s_load_dword %1, %4, %5 offset:0x400" \
                   : "=&s"(NXT), "=&s"(touch), "+v"(num), "+v"(den) \
                   : "s"(tabp), "s"(kb_nxt_s), "s"(kb_s), "i"(IMM) : "memory"); \
      else      asm volatile("s_load_dwordx16 %0, %4, %6 offset:%c7\n\t" QS_T4(0x0) QS_T4(0x100) "s_load_dword %1, %4, %5 offset:0x200\n\ts_load_dword %1, %4, %5 offset:0x240" \
                   : "=&s"(NXT), "=&s"(touch), "+v"(num), "+v"(den) \
                   : "s"(tabp), "s"(kb_nxt_s), "s"(kb_s), "i"(IMM) : "memory")
#define QS_LAND_T(NXT) asm volatile("s_waitcnt lgkmcnt(0)" : "+s"(NXT), "+s"(touch), "+v"(num), "+v"(den) : : "memory")
#define QS_H_SECTION(MODE) { \
        QS_ISSUE_K(WB, 64);  QS_ROWS_H_M(WA, 0, MODE) QS_LAND(WB); \
        QS_ISSUE_K(WA, 128); QS_ROWS_H_M(WB, 2, MODE) QS_LAND(WA); \
        QS_ISSUE_K(WB, 192); QS_ROWS_H_M(WA, 4, MODE) QS_LAND(WB); \
        QS_ISSUE_K(WA, 256); QS_ROWS_H_M(WB, 6, MODE) QS_LAND(WA); }
      if (md & QS_REC_H_ANY) {
        if (md & QS_REC_H_SKIP4) QS_H_SECTION(2)
        else if (md & QS_REC_H_EVEN) QS_H_SECTION(1)
        else QS_H_SECTION(0)
      }
      QS_ISSUE_T(WB, 320); QS_EDGE16(WA, 0) QS_LAND_T(WB);
      if (!DIAG && !(md & QS_REC_V_ANY)) { QS_ISSUE_R(WA, after_B); QS_EDGE16(WB, 16) QS_LAND_R(WA); }
      else                   { QS_ISSUE(WA, after_B);   QS_EDGE16(WB, 16) QS_LAND(WA); }
#define QS_V_SECTION(MODE) { \
        QS_ISSUE_K(WB, 448); QS_ROWS_V_M(WA, 0, 2, MODE) QS_LAND(WB); \
        QS_ISSUE_K(WA, 512); QS_ROWS_V_M(WB, 2, 2, MODE) QS_LAND(WA); \
        QS_ISSUE_K(WB, 576); QS_ROWS_V_M(WA, 4, 2, MODE) QS_LAND(WB); \
        if (!DIAG) { QS_ISSUE_R(WA, after_V); QS_ROWS_V_M(WB, 6, 1, MODE) QS_LAND_R(WA); } \
        else       { QS_ISSUE(WA, after_V);   QS_ROWS_V_M(WB, 6, 1, MODE) QS_LAND(WA); } }
      if (md & QS_REC_V_ANY) {
        if (md & QS_REC_V_SKIP4) QS_V_SECTION(2)
        else if (md & QS_REC_V_EVEN) QS_V_SECTION(1)
        else QS_V_SECTION(0)
      }
      if (DIAG) {
        QS_ISSUE_K(WB, 704);  QS_ROW_D(WA, 0) QS_LAND(WB);
        QS_ISSUE_K(WA, 768);  QS_ROW_D(WB, 1) QS_LAND(WA);
        QS_ISSUE_K(WB, 832);  QS_ROW_D(WA, 2) QS_LAND(WB);
        QS_ISSUE_K(WA, 896);  QS_ROW_D(WB, 3) QS_LAND(WA);
        QS_ISSUE_K(WB, 960);  QS_ROW_D(WA, 4) QS_LAND(WB);
        QS_ISSUE_K(WA, 1024); QS_ROW_D(WB, 5) QS_LAND(WA);
        QS_ISSUE_R(WB, next_first); QS_ROW_D(WA, 6) QS_LAND_R(WB);
        WA = WB;                 // 7 chunks: "a coefficient starts in WA" (landed: an ordinary copy)
      }
#undef QS_ROWS_H_M
#undef QS_HOISTED_TERM
#undef QS_ROWS_V_M
#undef QS_H_SECTION
#undef QS_V_SECTION
#undef QS_ISSUE
#undef QS_ISSUE_K
#undef QS_LAND
#undef QS_ISSUE_R
#undef QS_LAND_R
#undef QS_ISSUE_T
#undef QS_LAND_T
#undef QS_T4

      // ---- coefficient update (reference :1548-1564).  num'/den' = (num/den) * 2^-12: undo the scale (exact), round.
      __builtin_amdgcn_s_setprio(QS_PRIO_SLOW);
      // the coefficient is read from LDS BEFORE the division, so that the read's latency hides behind the ~20
      // instructions of the quotient instead of standing, waited for, right in front of the interval arithmetic
      lds_i16* const cptr = reinterpret_cast<lds_i16*>(reinterpret_cast<char*>(col) + lds_off);
      const int c0 = *cptr;
      const int r = f2i_x86(round_half_away((num / den) * 4096.0f));
      // Unconditional (for r == 0 this stores c0 back: c0 lies inside its own interval, which is what
      // the reference's `if (r)` leaves in place), so that `orig` is at hand for the two sums the
      // rebalance step needs (reference :1826-1833) -- they are integer sums, any order is exact, and
      // collecting them here saves the rebalance loop its 63 interval computations per block.
      {
        int orig, lo, hi;
        interval(c0, qk, x1k, x2k, orig, lo, hi);
        int v = (int)((uint32_t)c0 - (uint32_t)r);  // wraps like the x86 build
        v = min(max(v, lo), hi);
        if constexpr (DIAG) {
          *cptr = (lds_i16)v;
          chg |= (uint32_t)(v ^ c0);
          if (rebalance) {                            // wave-uniform
            reb_m0 += (long long)(v * orig);
            reb_m1 += (long long)(orig * orig);
          }
        } else {
          // The reference updates only `if (range)` (:1551).  Storing the clamped c0 back for r == 0 is the same thing
          // as long as c0 lies inside its own interval -- true for every coefficient a job can hold, but the reciprocal
          // tables divide exactly for |c| < 0x4000 only (:2527): beyond that the interval may miss c0 by one.  Such
          // coefficients also break what lets the rebalance sums be collected here -- that the stored value has the
          // `orig` of the value it replaced (inexact reciprocal, int16 wrap of the store).  A wave that was staged
          // with a coefficient outside [-0x2000, 0x2000) (big_wave; nothing below that can reach 0x4000) therefore
          // follows the reference to the letter, here and in the rebalance epilogue.
          // (a real, wave-uniform branch: the empty asm keeps hipcc from turning it into two selects on every wave's path)
          if (__builtin_expect(big_wave, 0)) { asm volatile("" : "+v"(v)); v = r ? v : c0; }
          *cptr = (lds_i16)v;
          chg_any |= __builtin_amdgcn_ballot_w64(v != c0);   // v_cmp + s_or_b64: no register per lane
          if (rebalance) {                            // wave-uniform; integer sums, exact in any order (24-bit operands)
            reb_a0 += (uint32_t)__mul24(v, orig);
            reb_a1 += (uint32_t)__mul24(orig, orig);
          }
        }
      }
      REC = RECN;   // landed by the coefficient's last step
      }             // (the branch of a coefficient that is not skipped)
    }
    kfirst = klast - 1;
    if (!DIAG && rebalance) {   // the anti-diagonal's partial sums go to LDS (wave-uniform)
      qs_lds_u64* const xreb = qs_xreb(col, lds, 0);
      qs_lds_add64(xreb, (long long)(unsigned long long)reb_a0);
      qs_lds_add64(xreb + 64, (long long)(unsigned long long)reb_a1);
      reb_a0 = 0; reb_a1 = 0;
    }
  }
  QS_SWAIT(WA);  // drain the last (unused) prefetch before the wave moves on

  // ---- rebalance (reference :1823-1848): scale AC energy back towards the
  // quantised original, inside each coefficient's interval.
  if (rebalance) {
    long long m0 = DIAG ? reb_m0 : (long long)*qs_xreb(col, lds, 0), m1 = DIAG ? reb_m1 : (long long)*qs_xreb(col, lds, 1);
    // A wave staged with a coefficient outside [-0x2000, 0x2000) (big_wave: never in a job) follows the reference to
    // the letter: the sums from the FINAL coefficients (:1826-1831), and below each `orig` as the JCOEF the reference
    // keeps it in (:1829: int16 wrap).  Everywhere else both are what the walk collected.
    const bool big = big_wave;
    if (big) {
      m0 = 0; m1 = 0;
#pragma unroll 1
      for (int n = 1; n < 64; ++n) {
        const int c = lds_coef(col, n);
        int orig, lo, hi;
        interval(c, cst->qn[n], cst->x1n[n], cst->x2n[n], orig, lo, hi);
        m0 += (long long)(c * orig);
        m1 += (long long)(orig * orig);
      }
    }
    if (m1 > m0) {
      const int mul = (int)(((m1 << 13) + (m0 >> 1)) / m0);
      // (luma walk) The hand-shaped form: one dword -- two coefficients -- per LDS read and write at an immediate offset
      // from the column pointer, the quantiser scalars through the scalar cache, 24-bit multiplies, and only the bound
      // that can bind (qs_rebalance_outward, qs_devfn.h: 13 VALU instructions per coefficient where the loop below
      // executes 20 and waits for three loads of its own; its listing shows 27, both forms of the bounds).  The
      // proof needs a wave without out-of-range coefficients and mul < 2^15.  Every such wave has mul <= 16384 -- each
      // term of m0 is v * orig >= orig^2 / 2, because |orig| >= div and |v - orig| <= div / 2 -- but the bound is
      // checked, not assumed: a wave with a larger mul in any rebalancing lane takes the loop below.
      bool outward = false;
      if constexpr (!DIAG) outward = !big && __builtin_amdgcn_ballot_w64((uint32_t)mul > (uint32_t)QS_REB_MUL_MAX) == 0;
      if (outward) {                                      // wave-uniform
        typedef const __attribute__((address_space(4))) int32_t* qs_cptr;   // wave-uniform, read-only: scalar loads
        const qs_cptr qn = (qs_cptr)(uintptr_t)cst->qn, x1n = (qs_cptr)(uintptr_t)cst->x1n, x2n = (qs_cptr)(uintptr_t)cst->x2n;
#pragma unroll
        for (int r = 0; r < 32; ++r) {
          const uint32_t d = col[r * QS_LDS_PITCH];
          const int c0 = (int16_t)(d & 0xffffu), c1 = (int32_t)d >> 16;
          const int v0 = r ? qs_rebalance_outward(c0, mul, qn[2 * r], x1n[2 * r], x2n[2 * r]) : c0;   // (DC stays)
          const int v1 = qs_rebalance_outward(c1, mul, qn[2 * r + 1], x1n[2 * r + 1], x2n[2 * r + 1]);
          col[r * QS_LDS_PITCH] = ((uint32_t)v0 & 0xffffu) | ((uint32_t)v1 << 16);
        }
      } else {
#pragma unroll 9
      for (int n = 1; n < 64; ++n) {
        const int c = lds_coef(col, n);
        int orig, lo, hi;
        interval(c, cst->qn[n], cst->x1n[n], cst->x2n[n], orig, lo, hi);
        if (big) {
          const int div = cst->qn[n], a = (int16_t)orig;
          hi = a + (a < 0 ? div >> 1 : (div - 1) >> 1);
          lo = a - (a > 0 ? div >> 1 : (div - 1) >> 1);
        }
        int v = (c * mul + 0x1000) >> 13;
        v = min(max(v, lo), hi);
        lds_set_coef(col, n, v);
      }
      }
    }
  }
  wave_lds_sync();

  // ---- write back, coalesced; optional final +-1023 clamp (reference :2680-2686)
  {
    // recompute the per-lane store addresses from an opaque copy of the lane
    // id, so that the 8 load addresses of the prologue do not stay live (and
    // get spilled) across the whole kernel
    // (luma walk: the lane id comes from mbcnt, so that not even the id itself stays live)
    int lane2 = DIAG ? lane : (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
    asm volatile("" : "+v"(lane2));
    const int lane = lane2;
    const int m0 = (lane & 7) * 4;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int idx = j * 64 + lane;
      const uint32_t* s = lds + m0 * QS_LDS_PITCH + (j * 8 + (lane >> 3));
      uint32_t d[4] = {s[0], s[QS_LDS_PITCH], s[2 * QS_LDS_PITCH], s[3 * QS_LDS_PITCH]};
      if (final_clamp) {
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          int lo = (int16_t)(d[c] & 0xffff), hi = (int32_t)d[c] >> 16;
          lo = min(max(lo, -1023), 1023); hi = min(max(hi, -1023), 1023);
          d[c] = ((uint32_t)lo & 0xffffu) | ((uint32_t)hi << 16);
        }
      }
      if (idx < nvec) gsrc[idx] = make_uint4(d[0], d[1], d[2], d[3]);
    }
  }

  // ---- fused pass A of the NEXT iteration (reference :2589-2620 of iteration n + 1): the block's final, unclamped
  // coefficients are still in this lane's LDS column, so their IDCT goes straight into the next iteration's pixel
  // plane -- a second plane, the other blocks of this launch still read `plane` -- together with the apron parts the
  // block owns.  One more IDCT per block-iteration (1.1 % of the kernel) instead of a separate launch that re-reads
  // every coefficient and, next to other work on the device, waits for free wave slots behind this very kernel.
#ifdef QS_SMOOTH_SET
  // (the plane's geometry is read again from the kernarg segment, through an opaque copy of the plane index, instead
  //  of staying live in five SGPRs across the coefficient walk, where the allocator would spill them into VGPR lanes)
  int pi2 = pi;
  asm volatile("" : "+s"(pi2));
  uint8_t* __restrict__ plane_next = set.ref[pi2].plane_next;
  const int rep = set.ref[pi2].mode, wblk2 = set.ref[pi2].wblk, hblk2 = set.ref[pi2].hblk, pitch2 = set.ref[pi2].pitch;
#else
  const int wblk2 = wblk, hblk2 = hblk, pitch2 = pitch;
#endif
  if (plane_next) {                                         // wave-uniform
    uint32_t ws[64];
    if constexpr (DIAG) lds_read_block_i16(col, ws); else lds_read_block_i16_1(col, ws);
    int lane3 = DIAG ? lane : (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));   // (as in the write-back)
    if constexpr (!DIAG) asm volatile("" : "+v"(lane3));
    if (base + lane3 < nblk)
      idct_ws_to_plane(ws, plane_next, wblk2, hblk2, pitch2, rep & QS_PLANE_REP_TOP, rep & QS_PLANE_REP_BOT, base + lane3);
  }
}

#undef QS_ROW_D
#undef QS_EDGE16
