// qs_smooth_dp_kernel.inc -- pass B for SMALL planes: one workgroup of NW waves per 64 blocks,
// the coefficients of a zigzag anti-diagonal spread over the waves ("diagonal-parallel").
//
// Why: with one block per lane (qs_smooth_kernel.inc) a block's 63 coefficient steps are one
// dependent chain of ~84 k (q3) / ~140 k (q4) instructions, and a wave gets one VALU issue slot
// per ~4.5 cycles however few waves share its SIMD -- a plane that leaves SIMDs with a single
// wave (a full-HD frame: 507 waves on 1024 SIMDs) takes 0.2 / 0.3 ms per iteration whatever its
// size.  But the reference only re-derives the block's pixels at the START of each of the 14
// anti-diagonals (reference quantsmooth.h:313-322, 1407-1409): the <= 8 coefficients of one
// anti-diagonal see the same pixels and write different coefficients, i.e. they do not depend on
// each other.  So NW waves take the same 64 blocks (lane l <-> block l in every wave), wave s
// processes coefficient kfirst - s, - s - NW, ... of the anti-diagonal, and the waves meet at a
// workgroup barrier per anti-diagonal; the coefficients live in ONE LDS copy per workgroup.
// Every wave still runs the exact serial sums of its coefficient with wave-uniform weights, so
// the arithmetic -- and the result -- is that of the one-block-per-lane kernel, bit for bit.
// The dependent chain shrinks to 14 refreshes + sum over anti-diagonals of ceil(len / NW)
// coefficient steps: 37 k instructions (NW = 4) instead of 84 k at q3.
// The refresh IDCT itself is shared between the waves through LDS, so the
// total work stays within ~1.2x of the one-block-per-lane kernel; the launcher picks this kernel
// for planes that cannot fill the chip otherwise (qs_kernels.hip: qs_dp_waves).
//
// Settings: QS_DP_KERNEL_NAME, QS_DP_SET (1: plane-set parameters), template <DIAG, NW>.
template <bool DIAG, int NW>
__global__ void __launch_bounds__(64 * NW, 3)
#ifdef QS_DP_SET
QS_DP_KERNEL_NAME(const QsPlaneSet set, int final_clamp) {
  const int gw = (int)blockIdx.x;                         // 64-block group of the set
  if (gw >= set.wave0[set.n]) return;                     // (workgroup-uniform)
  const int pi = qs_set_find(set, gw);
  const QsConsts* __restrict__ cst = set.ref[pi].cst;
  int16_t* __restrict__ coef = set.ref[pi].coef;
  const uint8_t* __restrict__ plane = set.ref[pi].plane;
  const int wblk = set.ref[pi].wblk, pitch = set.ref[pi].pitch;
  const int rebalance = set.ref[pi].mode & QS_PLANE_REBALANCE;
  const int nblk = wblk * set.ref[pi].hblk;
  const int base = (gw - set.wave0[pi]) * 64;
#else
QS_DP_KERNEL_NAME(const QsConsts* __restrict__ cst, int16_t* __restrict__ coef,
                  const uint8_t* __restrict__ plane, uint8_t* __restrict__ plane_next, int rep,
                  int wblk, int hblk, int pitch,
                  int rebalance, int final_clamp, int blk_begin, int blk_end) {
  const int nblk = blk_end;
  const int base = blk_begin + (int)blockIdx.x * 64;
#endif
  __shared__ uint32_t lds[32 * QS_LDS_PITCH];             // the 64 blocks' coefficients, one dword column per lane
  __shared__ long long reb_part[NW][64][2];               // per-wave partial sums of the rebalance step
  __shared__ uint32_t chg_sh[3];                          // "some block's coefficient changed in anti-diagonal g": slot (g + 1) % 3
  __shared__ uint32_t ws_sh[64 * 64];                     // shared IDCT workspace, then the 64 pixels, per lane
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  uint32_t* col = lds + lane;
  if (blockDim.x != 64 * NW) __builtin_trap();            // a launcher that pairs the wrong instantiation with the block size
  if (base >= nblk) return;                               // (workgroup-uniform: before any barrier)
  const int nvec = min(64, nblk - base) * 8;

  // ---- stage the 64 blocks (8 KiB contiguous), each wave its share of the eight 1 KiB slices
  uint4* gsrc = reinterpret_cast<uint4*>(coef) + (size_t)base * 8;
#ifdef QS_DP_SET
  // a plane whose coefficients are still quantised (QS_PLANE_QUANT, workgroup-uniform): dequantise on the way into LDS,
  // see qs_smooth_kernel.inc
  if (set.ref[pi].mode & QS_PLANE_QUANT) {
    const int m0 = (lane & 7) * 4;
    int q[8], unused = 0;
    qs_load_qraw8(cst, lane & 7, q);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      if (j % NW != wave) continue;
      const int idx = j * 64 + lane;
      uint4 v = make_uint4(0, 0, 0, 0);
      if (idx < nvec) v = gsrc[idx];
      v = qs_dequant8<false>(v, q, unused);
      uint32_t* dst = lds + m0 * QS_LDS_PITCH + (j * 8 + (lane >> 3));
      dst[0] = v.x; dst[QS_LDS_PITCH] = v.y; dst[2 * QS_LDS_PITCH] = v.z; dst[3 * QS_LDS_PITCH] = v.w;
    }
  } else
#endif
  {
    const int m0 = (lane & 7) * 4;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      if (j % NW != wave) continue;
      const int idx = j * 64 + lane;
      uint4 v = make_uint4(0, 0, 0, 0);
      if (idx < nvec) v = gsrc[idx];
      uint32_t* dst = lds + m0 * QS_LDS_PITCH + (j * 8 + (lane >> 3));
      dst[0] = v.x; dst[QS_LDS_PITCH] = v.y; dst[2 * QS_LDS_PITCH] = v.z; dst[3 * QS_LDS_PITCH] = v.w;
    }
  }
  // ---- neighbour edge pixels (every wave its own copy: 8 VGPRs), as in qs_smooth_kernel.inc
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
  if (threadIdx.x < 3) chg_sh[threadIdx.x] = 0;
  __syncthreads();

  constexpr int TS = DIAG ? 272 : 160;
  float px[64];   // own pixels * 2^-12
  float bd[32];   // own edge pixel minus neighbour pixel, * 2^-12 (top, bottom, left, right)
  const float* tabp = cst->tab;
  const int32_t* recp = &cst->rec[0][0];
  qs_w16 WA, WB;
  qs_i4 REC;
  long long reb_m0 = 0, reb_m1 = 0;
  int kfirst = 63;
  // The reference's need_refresh (quantsmooth.h:1407-1409, 1562), workgroup-uniform: the NW waves that share these 64
  // blocks publish "one of my coefficients changed a block" per anti-diagonal; when nobody did, the pixels (in ws_sh, and in
  // the registers of the waves that loaded them) are still those of the last refresh and the shared IDCT is skipped.
  // Three rotating LDS words: anti-diagonal g's writers use slot (g + 1) % 3 before the barrier that closes g, everybody
  // reads it after that barrier, and thread 0 clears slot (g + 2) % 3 (g + 1's writers', last read two barriers ago) meanwhile.
  uint32_t chg = 0;        // this wave: a coefficient of lane's block changed in the current anti-diagonal
  int gen = -1;            // anti-diagonal of the last refresh (the same in every wave)
  int my_gen = -2;         // ... whose pixels this wave holds in registers

#pragma unroll 1
  for (int g = 0; g < 14; ++g) {
    __builtin_amdgcn_s_setprio(QS_PRIO_SLOW);              // slow phases at raised wave priority, see qs_smooth_kernel.inc
    const int len = min(g + 1, 15 - g);
    const int klast = max(kfirst - len + 1, 1);
    // The refresh IDCT is shared: the NW waves hold the same 64 blocks, so each computes 8 / NW of the
    // 8 columns (pass 1) and of the 8 rows (pass 2) and the workspace travels through LDS -- two more
    // workgroup barriers per anti-diagonal, 3/4 of the IDCT instructions gone (NW = 4).  Integer
    // arithmetic with the same two descale points: identical pixels whoever computes them.
    const int stale = g == 0 ? 1 : __builtin_amdgcn_readfirstlane((int)chg_sh[g % 3]);   // (workgroup-uniform)
    if (threadIdx.x == 0) chg_sh[(g + 2) % 3] = 0;
    if (stale) gen = g;
    if (stale)
    {
#pragma unroll 1
      for (int cp = wave; cp < 4; cp += NW) {                  // column pair cp = block columns 2cp, 2cp + 1
        uint32_t ca[8], cb[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const uint32_t d = col[(j * 4 + cp) * QS_LDS_PITCH];
          ca[j] = (uint32_t)(int32_t)(int16_t)(d & 0xffff);
          cb[j] = (uint32_t)((int32_t)d >> 16);
        }
        idct8(ca, 1024u);
        idct8(cb, 1024u);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          ws_sh[(j * 8 + 2 * cp) * 64 + lane] = (uint32_t)((int32_t)ca[j] >> 11);
          ws_sh[(j * 8 + 2 * cp + 1) * 64 + lane] = (uint32_t)((int32_t)cb[j] >> 11);
        }
      }
      __syncthreads();
#pragma unroll 1
      for (int y = wave; y < 8; y += NW) {                     // rows: the pixels replace the workspace row in place
        uint32_t row[8]; float o[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) row[j] = ws_sh[(y * 8 + j) * 64 + lane];
        idct_pass2_row_f(row, o);
#pragma unroll
        for (int j = 0; j < 8; ++j) ws_sh[(y * 8 + j) * 64 + lane] = __builtin_bit_cast(uint32_t, o[j]);
      }
      __syncthreads();
    }
    // this wave has a coefficient on the anti-diagonal and does not hold the pixels of the last refresh yet
    // (it may have sat that anti-diagonal out: ws_sh keeps them until the next refresh)
    if (wave <= kfirst - klast && my_gen != gen) {
      my_gen = gen;
#pragma unroll
      for (int p = 0; p < 64; ++p) px[p] = __builtin_bit_cast(float, ws_sh[p * 64 + lane]);
#pragma unroll
      for (int e = 0; e < 8; ++e) asm volatile("" : "+v"(edge[e]));
#pragma unroll
      for (int x = 0; x < 8; ++x) {
        bd[x]      = px[x]         - pix_from_byte(edge[0 + (x >> 2)], x & 3);
        bd[8 + x]  = px[56 + x]    - pix_from_byte(edge[2 + (x >> 2)], x & 3);
        bd[16 + x] = px[x * 8]     - pix_from_byte(edge[4 + (x >> 2)], x & 3);
        bd[24 + x] = px[x * 8 + 7] - pix_from_byte(edge[6 + (x >> 2)], x & 3);
      }
    }
#pragma unroll 1
    for (int k = kfirst - wave; k >= klast; k -= NW) {
#pragma unroll
      for (int p = 0; p < 64; ++p) asm volatile("" : "+v"(px[p]));   // keep the pixel differences inside the loop
      // the coefficient's record and BOTH candidates for its first weight chunk (the H section's
      // first rows, or the border section when the coefficient has no horizontal frequency) in one
      // statement that ends with the wait: nothing is in flight behind it
      const uint32_t kb = (uint32_t)k * (TS * 4);
      asm volatile("s_load_dwordx4 %0, %3, %4\n\ts_load_dwordx16 %1, %5, %6\n\ts_load_dwordx16 %2, %5, %7\n\ts_waitcnt lgkmcnt(0)"
                   : "=&s"(REC), "=&s"(WA), "=&s"(WB)
                   : "s"(recp), "s"((uint32_t)__builtin_amdgcn_readfirstlane(k * 16)), "s"(tabp),
                     "s"((uint32_t)__builtin_amdgcn_readfirstlane((int)kb)), "s"((uint32_t)__builtin_amdgcn_readfirstlane((int)(kb + 256u)))
                   : "memory");
      // what depends on k alone comes ready-made in the record's fourth dword (qs_device.h: QS_REC_*), as in qs_smooth_kernel.inc
      const int md = REC[3];
      const int x2k = (REC[0] >> 16) & 31, qk = REC[1] & 0xffff, x1k = REC[1] >> 16;
      const uint32_t lds_off = ((uint32_t)md >> QS_REC_LDS_SHIFT) & 0x3fffu;
      int rs_bits = REC[2];                      // (opaque copy: see the sub-register hazard in qs_smooth_kernel.inc)
      asm volatile("" : "+s"(rs_bits));
      const float Rs = __builtin_bit_cast(float, rs_bits);   // 2q * 2^-12
#if QS_Q1_SKIP
      if (md & QS_REC_Q1) {                      // quantiser 1: nothing can change, see qs_smooth_kernel.inc
        if (rebalance) {
          const int c0 = *reinterpret_cast<lds_i16*>(reinterpret_cast<char*>(col) + lds_off);
          reb_m0 += (long long)(c0 * c0);
          reb_m1 += (long long)(c0 * c0);
        }
        continue;
      }
#endif
      if (!(md & QS_REC_H_ANY)) WA = WB;         // no H section: the border chunk comes first
      const uint32_t after_V = DIAG ? kb + 640u : kb;        // (the last step's fetch is a dummy here)
      const uint32_t after_B = (md & QS_REC_V_ANY) ? kb + 384u : after_V;
      float num = 0.0f, den = 0.0f;
      __builtin_amdgcn_s_setprio(QS_PRIO_TERMS);
      // the optional terms test these (s_cmp_lg_u32 against 0): non-zero = the term's weight is structurally zero
      const int h_skip4 = md & QS_REC_H_SKIP4, h_even = md & QS_REC_H_EVEN;
      const int v_skip4 = md & QS_REC_V_SKIP4, v_even = md & QS_REC_V_EVEN;
      (void)h_skip4; (void)h_even; (void)v_skip4; (void)v_even;

#define QS_ROWS_H(W, Y0) { \
        _Pragma("unroll") for (int yy = 0; yy < 2; ++yy) \
        _Pragma("unroll") for (int x = 0; x < 7; ++x) { \
          if (x == 3) QS_TERM_OPT(h_even, px[((Y0) + yy) * 8 + x], px[((Y0) + yy) * 8 + x + 1], W[yy * 8 + x]) \
          else if (x & 1) QS_TERM_OPT(h_skip4, px[((Y0) + yy) * 8 + x], px[((Y0) + yy) * 8 + x + 1], W[yy * 8 + x]) \
          else QS_TERM(px[((Y0) + yy) * 8 + x], px[((Y0) + yy) * 8 + x + 1], W[yy * 8 + x]) } }
#define QS_ROWS_V(W, Y0, NY) { \
        _Pragma("unroll") for (int yy = 0; yy < (NY); ++yy) \
        _Pragma("unroll") for (int x = 0; x < 8; ++x) { \
          if ((Y0) + yy == 3) QS_TERM_OPT(v_even, px[((Y0) + yy) * 8 + x], px[((Y0) + yy) * 8 + x + 8], W[yy * 8 + x]) \
          else if (((Y0) + yy) & 1) QS_TERM_OPT(v_skip4, px[((Y0) + yy) * 8 + x], px[((Y0) + yy) * 8 + x + 8], W[yy * 8 + x]) \
          else QS_TERM(px[((Y0) + yy) * 8 + x], px[((Y0) + yy) * 8 + x + 8], W[yy * 8 + x]) } }
#define QS_ROW_D(W, Y) { \
        _Pragma("unroll") for (int x = 0; x < 7; ++x) { \
          QS_TERM(px[(Y) * 8 + x], px[(Y) * 8 + x + 9], W[x]) \
          QS_TERM(px[(Y) * 8 + x + 1], px[(Y) * 8 + x + 8], W[8 + x]) } }
#define QS_EDGE16(W, J0) { \
        _Pragma("unroll") for (int j = 0; j < 16; ++j) QS_TERM_D(bd[(J0) + j], W[j]) }
      // landed pipeline (see qs_smooth_kernel.inc): issue the next chunk, 14-16 terms, wait
#define QS_ISSUE(NXT, BYTEOFF) \
      asm volatile("s_load_dwordx16 %0, %3, %4" : "=&s"(NXT), "+v"(num), "+v"(den) \
                   : "s"(tabp), "s"((uint32_t)__builtin_amdgcn_readfirstlane((int)(BYTEOFF))) : "memory")
      // (a chunk of the current row: base + row-offset SGPR + immediate, see qs_smooth_kernel.inc)
#define QS_ISSUE_K(NXT, IMM) \
      asm volatile("s_load_dwordx16 %0, %3, %4 offset:%c5" : "=&s"(NXT), "+v"(num), "+v"(den) \
                   : "s"(tabp), "s"(kb_s), "i"(IMM) : "memory")
#define QS_LAND(NXT) asm volatile("s_waitcnt lgkmcnt(0)" : "+s"(NXT), "+v"(num), "+v"(den) : : "memory")
      const uint32_t kb_s = (uint32_t)__builtin_amdgcn_readfirstlane((int)kb);
      if (md & QS_REC_H_ANY) {
        QS_ISSUE_K(WB, 64);  QS_ROWS_H(WA, 0) QS_LAND(WB);
        QS_ISSUE_K(WA, 128); QS_ROWS_H(WB, 2) QS_LAND(WA);
        QS_ISSUE_K(WB, 192); QS_ROWS_H(WA, 4) QS_LAND(WB);
        QS_ISSUE_K(WA, 256); QS_ROWS_H(WB, 6) QS_LAND(WA);
      }
      QS_ISSUE_K(WB, 320);   QS_EDGE16(WA, 0) QS_LAND(WB);
      QS_ISSUE(WA, after_B);     QS_EDGE16(WB, 16) QS_LAND(WA);
      if (md & QS_REC_V_ANY) {
        QS_ISSUE_K(WB, 448); QS_ROWS_V(WA, 0, 2) QS_LAND(WB);
        QS_ISSUE_K(WA, 512); QS_ROWS_V(WB, 2, 2) QS_LAND(WA);
        QS_ISSUE_K(WB, 576); QS_ROWS_V(WA, 4, 2) QS_LAND(WB);
        QS_ISSUE(WA, after_V);   QS_ROWS_V(WB, 6, 1) QS_LAND(WA);
      }
      if (DIAG) {
        QS_ISSUE_K(WB, 704);  QS_ROW_D(WA, 0) QS_LAND(WB);
        QS_ISSUE_K(WA, 768);  QS_ROW_D(WB, 1) QS_LAND(WA);
        QS_ISSUE_K(WB, 832);  QS_ROW_D(WA, 2) QS_LAND(WB);
        QS_ISSUE_K(WA, 896);  QS_ROW_D(WB, 3) QS_LAND(WA);
        QS_ISSUE_K(WB, 960);  QS_ROW_D(WA, 4) QS_LAND(WB);
        QS_ISSUE_K(WA, 1024); QS_ROW_D(WB, 5) QS_LAND(WA);
        QS_ISSUE(WB, kb);         QS_ROW_D(WA, 6) QS_LAND(WB);
      }
#undef QS_ISSUE
#undef QS_ISSUE_K
#undef QS_LAND
#undef QS_ROWS_H
#undef QS_ROWS_V
#undef QS_ROW_D
#undef QS_EDGE16

      // coefficient update (reference :1548-1564) + the rebalance step's sums, as in qs_smooth_kernel.inc;
      // every wave writes a different coefficient of the shared column
      __builtin_amdgcn_s_setprio(QS_PRIO_SLOW);
      lds_i16* const cptr = reinterpret_cast<lds_i16*>(reinterpret_cast<char*>(col) + lds_off);
      const int c0 = *cptr;                      // (read before the division: its LDS latency hides behind the quotient)
      const int r = f2i_x86(round_half_away((num / den) * 4096.0f));
      {
        int orig, lo, hi;
        interval(c0, qk, x1k, x2k, orig, lo, hi);
        int v = (int)((uint32_t)c0 - (uint32_t)r);  // wraps like the x86 build
        v = min(max(v, lo), hi);
        *cptr = (lds_i16)v;
        chg |= (uint32_t)(v ^ c0);
        if (rebalance) {
          reb_m0 += (long long)(v * orig);
          reb_m1 += (long long)(orig * orig);
        }
      }
    }
    kfirst = klast - 1;
    if (__builtin_amdgcn_ballot_w64(chg != 0) != 0 && lane == 0) chg_sh[(g + 1) % 3] = 1;   // (several waves may store the same 1)
    chg = 0;
    __syncthreads();                       // the anti-diagonal's coefficients are in LDS for everybody's next refresh
  }

  // ---- rebalance (reference :1823-1848): the waves' partial sums meet in LDS, every wave forms the
  // totals (integer sums: any order is exact) and rescales its share of the 63 coefficients
  if (rebalance) {
    reb_part[wave][lane][0] = reb_m0;
    reb_part[wave][lane][1] = reb_m1;
    __syncthreads();
    long long m0 = 0, m1 = 0;
#pragma unroll
    for (int w = 0; w < NW; ++w) { m0 += reb_part[w][lane][0]; m1 += reb_part[w][lane][1]; }
    if (m1 > m0) {
      const int mul = (int)(((m1 << 13) + (m0 >> 1)) / m0);
#pragma unroll 1
      for (int n = 1 + wave; n < 64; n += NW) {
        const int c = lds_coef(col, n);
        int orig, lo, hi;
        interval(c, cst->qn[n], cst->x1n[n], cst->x2n[n], orig, lo, hi);
        int v = (c * mul + 0x1000) >> 13;
        v = min(max(v, lo), hi);
        lds_set_coef(col, n, v);
      }
    }
    __syncthreads();
  }

  // ---- write back, coalesced, each wave its slices; optional final +-1023 clamp (reference :2680-2686)
  {
    const int m0 = (lane & 7) * 4;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      if (j % NW != wave) continue;
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

  // ---- fused pass A of the next iteration (see qs_smooth_kernel.inc): the shared IDCT once more, on the final, unclamped
  // coefficients in LDS -- the waves split the column pairs of pass 1 and the rows of pass 2 as in the refresh -- and each
  // wave stores its pixel rows of all 64 blocks into the NEXT plane (every lane of a wave a different block: the 8-byte
  // row stores of a wave are 512 contiguous bytes, as in pass A).
#ifdef QS_DP_SET
  uint8_t* __restrict__ plane_next = set.ref[pi].plane_next;
  const int rep = set.ref[pi].mode, hblk = set.ref[pi].hblk;
#endif
  if (plane_next) {                                          // (workgroup-uniform)
#pragma unroll 1
    for (int cp = wave; cp < 4; cp += NW) {
      uint32_t ca[8], cb[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const uint32_t d = col[(j * 4 + cp) * QS_LDS_PITCH];
        ca[j] = (uint32_t)(int32_t)(int16_t)(d & 0xffff);
        cb[j] = (uint32_t)((int32_t)d >> 16);
      }
      idct8(ca, 1024u);
      idct8(cb, 1024u);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        ws_sh[(j * 8 + 2 * cp) * 64 + lane] = (uint32_t)((int32_t)ca[j] >> 11);
        ws_sh[(j * 8 + 2 * cp + 1) * 64 + lane] = (uint32_t)((int32_t)cb[j] >> 11);
      }
    }
    __syncthreads();
    const int b = min(base + lane, nblk - 1);
    const int by2 = b / wblk, bx2 = b - by2 * wblk;
    uint8_t* org2 = plane_next + (size_t)(by2 * 8 + 1) * pitch + QS_APRON_X + bx2 * 8;
#pragma unroll 1
    for (int y = wave; y < 8; y += NW) {
      uint32_t row[8]; int o[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) row[j] = ws_sh[(y * 8 + j) * 64 + lane];
      idct_pass2_row(row, o);
      if (base + lane < nblk)
        store_pixel_row(org2, pitch, y, o, bx2, by2, wblk, hblk, rep & QS_PLANE_REP_TOP, rep & QS_PLANE_REP_BOT);
    }
  }
}
