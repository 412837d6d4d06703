// qs_encode.h -- the device entropy coder (qs_hip_encode_device_batch, csrc/qs_kernels_encode.hip): what the kernels
// and the host driver (csrc/qs_encode_job.cpp) share.  The output is the entropy-coded segment of one baseline
// sequential Huffman scan as libjpeg 9 (jchuff.c behind jpeg_write_coefficients) writes it: DESIGN.md section 13.
#pragma once
#include <stdint.h>

#define QS_ENC_CHUNK 32            // jobs per launch set (their addresses travel in the kernel arguments, 3.1 KiB)
#define QS_ENC_WG 256              // lanes per workgroup = scan blocks per workgroup of the sizing and emit kernels
// longest code of one block: DC 16 + 11 bits, 63 AC of 16 + 10 bits
#define QS_ENC_MAXBITS (27 + 63 * 26)
// words the emit kernel stages per workgroup: 256 blocks of QS_ENC_MAXBITS behind up to 31 bits of the word they start in
#define QS_ENC_LDS_WORDS ((31 + QS_ENC_WG * QS_ENC_MAXBITS + 31) / 32)
// the restart variant: every lane can own an interval end, whose padding adds up to 7 bits to the workgroup's image
#define QS_ENC_LDS_WORDS_RST (QS_ENC_LDS_WORDS + (7 * QS_ENC_WG + 31) / 32)
#define QS_ENC_SCHUNK 4096         // bytes of the unstuffed stream per stuffing step (16 per lane)
#define QS_ENC_CODES (2 * 16 + 2 * 256)   // code words of one job: dc[2][16], ac[2][256]
#define QS_ENC_SWG_MAX 1024        // workgroups a job's stuffing kernels get at most (they stride over the chunks)

// status bits collected per job while it runs (QsEncState.flags); the caller sees 1, 3 or 2 in this order of precedence
// (4, before all of them: descriptors with a restart interval under the kernels without -- QsEncArgs.restart)
#define QS_ENC_F_BADCOEF 1u
#define QS_ENC_F_NOCODE 2u

// the scan of one geometry: how scan block b maps to a component and a block of its array
struct QsEncGeom {
  int32_t ncomp;
  int32_t nw[4], nh[4];            // libjpeg's width_in_blocks / height_in_blocks: the blocks that exist
  int32_t stride[4];               // row stride of the array in blocks
  int32_t hs[4], vs[4];            // blocks per MCU across / down (1 x 1 in a one-component scan)
  int32_t first[4];                // index of the component's first block inside an MCU
  int32_t slot[4];                 // which of QsEncPtrs.coef holds the component
  int32_t mcus_x, mcus, bpm;       // MCUs per row, MCUs in the scan, blocks per MCU
  int32_t nblocks;                 // mcus * bpm
};

// why qs_enc_geometry refuses a scan
#define QS_GEOM_OK 0
#define QS_GEOM_ARGS 1             // components not 1..4, or an image outside 1..65500
#define QS_GEOM_SHORT 2            // *detail = the first component whose array is short of nw x nh blocks (both filled in)
#define QS_GEOM_MCU 3              // *detail = the blocks of an MCU, more than libjpeg's 10
#define QS_GEOM_SCAN 4             // more than 0x7fff0000 blocks in the scan

#if defined(__HIPCC__) || defined(__HIP__)
#define QS_ENC_HD __host__ __device__ static inline   // (static: the library exports nothing from here)
#else
#define QS_ENC_HD static inline
#endif

// The scan that carries all components of a frame (jcmaster.c / jdinput.c per_scan_setup), for the coder and the scan
// reader alike (csrc/qs_read.h: qr_geometry).  hs / vs: the sampling factors, which the caller has checked; stride /
// rows: the arrays in blocks; slot: null means slot[c] = c.  -> QS_GEOM_*
QS_ENC_HD int qs_enc_geometry(int ncomp, int W, int H, const int32_t* hs, const int32_t* vs, const int32_t* stride,
                              const int32_t* rows, const int32_t* slot, QsEncGeom* g, int* detail) {
  *g = QsEncGeom();
  if (ncomp < 1 || ncomp > 4 || W < 1 || H < 1 || W > 65500 || H > 65500) return QS_GEOM_ARGS;
  int mh = 1, mv = 1;
  for (int c = 0; c < ncomp; ++c) {
    if (hs[c] > mh) mh = hs[c];
    if (vs[c] > mv) mv = vs[c];
  }
  g->ncomp = ncomp;
  for (int c = 0; c < ncomp; ++c) {
    g->nw[c] = (int32_t)(((long long)W * hs[c] + 8LL * mh - 1) / (8LL * mh));   // width_in_blocks / height_in_blocks
    g->nh[c] = (int32_t)(((long long)H * vs[c] + 8LL * mv - 1) / (8LL * mv));
    g->stride[c] = stride[c];
    g->slot[c] = slot ? slot[c] : c;
    if (stride[c] < g->nw[c] || rows[c] < g->nh[c]) {
      *detail = c;
      return QS_GEOM_SHORT;
    }
  }
  if (ncomp == 1) {                                                 // non-interleaved: an MCU is one block
    g->hs[0] = g->vs[0] = 1;
    g->bpm = 1;
    g->mcus_x = g->nw[0];
    g->mcus = g->nw[0] * g->nh[0];
  } else {
    int first = 0;
    for (int c = 0; c < ncomp; ++c) {
      g->hs[c] = hs[c];
      g->vs[c] = vs[c];
      g->first[c] = first;
      first += hs[c] * vs[c];
    }
    if (first > 10) {
      *detail = first;
      return QS_GEOM_MCU;
    }
    g->bpm = first;
    g->mcus_x = (int32_t)((W + 8LL * mh - 1) / (8LL * mh));
    const long long mcus = (long long)g->mcus_x * ((H + 8LL * mv - 1) / (8LL * mv));
    if (mcus * first > 0x7fff0000LL) return QS_GEOM_SCAN;
    g->mcus = (int32_t)mcus;
  }
  g->nblocks = g->mcus * g->bpm;
  return QS_GEOM_OK;
}

// One job as the kernels see it (workspace, written by prepare): geometry, code tables and where its scratch arrays
// lie in the workspace.  No addresses of caller memory.
struct QsEncJob {
  QsEncGeom g[2];                  // variant 0 (d_stop 0: replacement chroma when the job has it), variant 1
  int32_t two;                     // 1: the variant follows d_stop[job]
  int32_t tbl[4];                  // Huffman table (0 / 1) of each component
  int32_t wg0, nwg;                // sizing / emit workgroups of this job in its chunk's launches
  int32_t swg0, nswg;              // the same for the stuffing kernels
  int32_t ri[2];                   // restart interval of each variant in MCUs; 0: none (also when it covers the scan)
  int32_t pad;
  uint64_t off_bits;               // uint16[nwg * 256]: code length of each scan block
  uint64_t off_wgsum;              // uint32[nwg]: bits of each workgroup's blocks
  uint64_t off_wgoff;              // uint64[nwg]: their exclusive scan
  uint64_t off_raw, raw_cap;       // the unstuffed stream (bytes), its capacity
  uint64_t off_ffcnt;              // uint32[raw_cap / QS_ENC_SCHUNK]: 0xFF bytes per stuffing chunk
  uint64_t off_ffoff;              // uint64[...]: their exclusive scan
  uint64_t off_state;              // QsEncState
  // restart intervals (used by the restart kernels only; an interval = ri MCUs, the whole scan where ri is 0)
  uint64_t off_rrel;               // uint32[intervals]: bits of the workgroup's blocks before the interval's first block
  uint64_t off_rd;                 // uint64[intervals + 1]: padding bits of all intervals before this one
  uint64_t off_rp;                 // uint64[intervals + 1]: the byte of the unstuffed stream the interval starts at
  uint32_t dc[2][16];              // (size << 16) | code by category; size 0 = the table has no such symbol
  uint32_t ac[2][256];             // the same by run/size symbol
};

struct QsEncState {
  uint64_t total_bits;             // of the unstuffed stream (restart kernels: the interval paddings included)
  uint64_t raw_bytes;              // ceil(total_bits / 8)
  uint32_t flags;                  // QS_ENC_F_*
  uint32_t dead;                   // 1: flags were set when the scan ran; the later kernels leave the job alone
  uint32_t nchunks, pad;
};

struct QsEncPtrs {
  const int16_t* coef[6];          // 0..3 variant 0's arrays; 4..5 variant 1's chroma (component 0 is coef[0] in both)
  int32_t nblk[6];                 // blocks in each array: the kernels bound every read by them
  uint8_t* out;
  uint64_t cap;                    // bytes the caller's buffer holds
};
struct QsEncArgs {
  const QsEncJob* jobs;            // the chunk's descriptors (workspace)
  uint8_t* ws;                     // the workspace base the descriptors' offsets refer to
  const int32_t* d_stop;           // the caller's int32[njobs] or null, indexed by job0 + i
  uint64_t* d_len;                 // indexed by job0 + i
  int32_t* d_status;
  uint32_t* d_counts;              // histogram run: uint32[njobs][4][257], else null
  int32_t job0, n;
  int32_t restart;                 // 1: the restart instantiations run (else a job with an interval ends with status 4)
  // the whole-file run (qs_hip_encode_device_batch_files, csrc/qs_kernels_huff.hip); all null / 0 in every other run
  const uint32_t* codes;           // scratch: uint32[njobs][QS_ENC_CODES] -- the table kernel's code words instead of the
                                   // descriptors' (dc[2][16] then ac[2][256], the same form); null: the descriptors'
  uint64_t* prefix;                // scratch: uint64[njobs] -- bytes of the file in front of the segment; null: 0
  const int32_t* tstatus;          // scratch: int32[njobs] -- not 0: a table of the job has a code length above 32 (status 5)
  uint32_t tail;                   // bytes of the file behind the segment (EOI)
  uint32_t fixed[QS_ENC_CHUNK][2]; // head + mid bytes of each variant: what qe_init makes the prefix when `codes` is null
                                   // (with `codes` the table kernel wrote it: the DHT markers' bytes come on top)
  int32_t wg0[QS_ENC_CHUNK];       // each job's first workgroup in the block kernels' launch (QsEncJob.wg0) ...
  int32_t swg0[QS_ENC_CHUNK];      // ... and in the stuffing kernels': a workgroup finds its job without touching memory
  QsEncPtrs p[QS_ENC_CHUNK];
};

// ---- the whole-file run: optimal tables and framing (csrc/qs_kernels_huff.hip) ----
#define QS_ENC_TABLE_BYTES 273     // sizeof(qs_hip_huff_table): bits[17], huffval[256]
#define QS_ENC_TABLES_BYTES (4 * QS_ENC_TABLE_BYTES + 4)   // sizeof(qs_hip_huff_tables): dc[2], ac[2], has_dc[2], has_ac[2]
#define QS_ENC_DHT_MAX (4 * (5 + 16 + 256))                 // the DHT markers of one job at most

// the caller's memory of one job of the whole-file run
struct QsFramePtrs {
  const uint8_t* head[2];          // per variant: SOI .. SOF (without optimize: .. the DHT markers); null with 0 bytes
  const uint8_t* mid[2];           // [DRI] SOS header
  uint32_t head_bytes[2], mid_bytes[2];
  uint8_t* out;
  uint64_t cap;
};
// arguments of the table kernel (qh_tables) and the framing kernel (qh_frame), per chunk of jobs
struct QsHuffArgs {
  const QsEncJob* jobs;            // the chunk's descriptors (workspace)
  const int32_t* d_stop;
  const uint32_t* counts;          // scratch: uint32[njobs][4][257], indexed by job0 + i like everything below
  uint32_t* codes;                 // scratch: uint32[njobs][QS_ENC_CODES]
  uint8_t* tables;                 // scratch: qs_hip_huff_tables[njobs]
  uint8_t* d_tables;               // the caller's qs_hip_huff_tables[njobs] or null
  uint64_t* prefix;                // scratch: uint64[njobs]
  int32_t* tstatus;                // scratch: int32[njobs]
  const uint64_t* d_len;
  const int32_t* d_status;
  int32_t job0, n;
  int32_t optimize, framed;        // framed 0: no head, mid or EOI (frames == NULL)
  QsFramePtrs f[QS_ENC_CHUNK];
};
