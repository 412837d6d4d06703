// qs_encode_job.cpp -- the device entropy coder of the flat C ABI (include/jpegqs_hip.h):
// qs_hip_encode_device_batch_info[_opts] / _prepare[_opts] / qs_hip_encode_device_batch / _histogram, and the host-only
// qs_hip_huff_optimal / qs_hip_huff_standard.  What libjpeg 9 writes between the SOS header and EOI for
// jpeg_write_coefficients on the arrays of qs_hip_job records (no scan script, 8 bits; restart intervals through the
// _opts calls), computed on the device (qs_kernels_encode.hip).
// qs_hip_encode_device_batch_files is the same run with the optimal tables made on the device and the file's markers
// around the segment (qs_kernels_huff.hip): it shares enqueue() with the plain run and keeps its
// own arrays in the caller's scratch, never in the workspace.  qs_hip_huff_optimal[_device]: csrc/qs_huff.h.
//
// Workspace: the QsEncJob descriptors of the batch, then per job the arrays of one coded scan (csrc/qs_encode_plan.h, with
// the restart rule, the scratch and the registry of prepared workspaces) -- a function of the jobs' geometry and restart
// options alone; the code tables in the descriptors come from prepare's `tables`.  The run calls describe the batch
// again and take from the registry only the batch size, which launch chunks hold a restart job and how large the
// workspace must be.  A workspace they do not find there runs as one without restart jobs, as every workspace did before
// there were options; should its descriptors hold an interval after all, the kernels end those jobs with status 4.
#include "qs_common.h"
#include "qs_stage.h"
#include "qs_encode.h"
#include "qs_huff.h"
#include "qs_encode_prog.h"
#include "qs_encode_plan.h"

#include <algorithm>

void qs_launch_encode(const QsEncArgs& a, int wgs, int swgs, bool restart, hipStream_t s);
void qs_launch_huff_optimal(const uint32_t* d_counts, int ntables, uint8_t* d_tables, int32_t* d_status, hipStream_t s);
void qs_launch_huff_tables(const QsHuffArgs& a, hipStream_t s);
void qs_launch_huff_frame(const QsHuffArgs& a, hipStream_t s);

static_assert(sizeof(qs_hip_huff_table) == QS_ENC_TABLE_BYTES && sizeof(qs_hip_huff_tables) == QS_ENC_TABLES_BYTES,
              "the kernels address the tables by these sizes");
static_assert(sizeof(QsEncArgs) <= 4096 && sizeof(QsHuffArgs) <= 4096, "kernel arguments: 4 KiB at most");

namespace {

// JPEG Annex K.3 (the tables libjpeg installs with jpeg_set_defaults): [0] luminance, [1] chrominance
const uint8_t STD_DC_BITS[2][17] = {{0, 0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0},
                                    {0, 0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}};
const uint8_t STD_AC_BITS[2][17] = {{0, 0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d},
                                    {0, 0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77}};
const uint8_t STD_AC_VAL[2][162] = {
    {0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81,
     0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18,
     0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48,
     0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75,
     0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99,
     0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3,
     0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5,
     0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa},
    {0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08,
     0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25,
     0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47,
     0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74,
     0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97,
     0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba,
     0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4,
     0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa}};

void standard_table(int is_ac, int tbl, qs_hip_huff_table* t) {
  memset(t, 0, sizeof *t);
  if (is_ac) {
    memcpy(t->bits, STD_AC_BITS[tbl], 17);
    memcpy(t->huffval, STD_AC_VAL[tbl], 162);
  } else {
    memcpy(t->bits, STD_DC_BITS[tbl], 17);
    for (int i = 0; i < 12; ++i) t->huffval[i] = (uint8_t)i;
  }
}

// jpeg_make_c_derived_tbl of jchuff.c: (size << 16) | code per symbol, 0 where the table has none
int derive(const qs_hip_huff_table& t, bool is_dc, uint32_t* out, int nout, const char* who, const char* what) {
  for (int i = 0; i < nout; ++i) out[i] = 0;
  int p = 0;
  uint32_t code = 0;
  for (int l = 1; l <= 16; ++l) {
    for (int i = 0; i < t.bits[l]; ++i, ++p, ++code) {
      if (p >= 256 || code >= (1u << l)) return qs_fail(QS_HIP_EINVAL, "%s: %s is not a valid Huffman table", who, what);
      const int sym = t.huffval[p];
      if ((is_dc && sym > 15) || out[sym % nout])
        return qs_fail(QS_HIP_EINVAL, "%s: %s has a bad or repeated symbol 0x%02x", who, what, sym);
      out[sym] = ((uint32_t)l << 16) | code;
    }
    code <<= 1;
  }
  return QS_HIP_OK;
}

// one geometry: the sampling factors hs / vs, array strides and slots of its components
// any_mcu: the caller codes the frame scan by scan (the progressive run) -- more than 10 blocks in the frame's MCU are its
// to judge per scan, and the geometry comes back with the frame's MCU grid
int geometry(const qs_hip_job* job, const int* hs, const int* vs, const int* stride, const int* rows, const int* slot,
             QsEncGeom* g, const char* who, bool any_mcu = false) {
  const int W = job->image_width, H = job->image_height;
  int d = 0;
  switch (qs_enc_geometry(job->ncomp, W, H, hs, vs, stride, rows, slot, g, &d)) {
    case QS_GEOM_OK: return QS_HIP_OK;
    case QS_GEOM_SHORT:
      return qs_fail(QS_HIP_EINVAL, "%s: component %d has %d x %d blocks, a %d x %d image sampled %dx%d needs %d x %d", who, d,
                     stride[d], rows[d], W, H, hs[d], vs[d], g->nw[d], g->nh[d]);
    case QS_GEOM_MCU:
      if (any_mcu) {
        qp_complete_frame(W, H, d, g);
        return QS_HIP_OK;
      }
      return qs_fail(QS_HIP_ENOTSUP, "%s: %d blocks in an MCU; libjpeg takes at most 10", who, d);
    case QS_GEOM_SCAN: return qs_fail(QS_HIP_EINVAL, "%s: more than 2^31 blocks in the scan", who);
    default: return qs_fail(QS_HIP_EINVAL, "%s: bad job", who);      // (describe has looked at ncomp and the image)
  }
}

int describe(const qs_hip_job* job, QsEncJob* D, QsEncPtrs* P, bool need_arrays, qs_hip_encode_info* info, const char* who,
             bool any_mcu = false) {
  if (int r = check_job(job, who)) return r;
  const int n = job->ncomp;
  if (job->image_width <= 0 || job->image_height <= 0 || job->image_width > 65500 || job->image_height > 65500)
    return qs_fail(QS_HIP_EINVAL, "%s: the encoder needs image_width x image_height within 65500 (got %d x %d)", who,
                   job->image_width, job->image_height);
  memset(D, 0, sizeof *D);
  if (P) memset(P, 0, sizeof *P);
  // jpeg_set_colorspace: table 1 for the chroma of YCbCr and YCCK, table 0 for everything else
  const int cs = job->colorspace;
  const int need = cs == 1 ? 1 : (cs == 2 || cs == 3) ? 3 : (cs == 4 || cs == 5) ? 4 : 0;
  if (need != n)
    return qs_fail(QS_HIP_ENOTSUP, "%s: %d components in colour space %d: the encoder covers grayscale (1), RGB and YCbCr (3), "
                   "CMYK and YCCK (4)", who, n, cs);
  for (int c = 0; c < n; ++c) {
    D->tbl[c] = ((cs == 3 || cs == 5) && (c == 1 || c == 2)) ? 1 : 0;
    if (int r = check_sampling(job, c, who)) return r;
    if (job->wblk[c] < 1 || job->hblk[c] < 1) return qs_fail(QS_HIP_EINVAL, "%s: component %d has no blocks", who, c);
  }
  const bool up = job->up_wblk > 0 && n == 3;
  int hs[4], vs[4], stride[4], rows[4], slot[4];
  for (int v = 0; v < (up ? 2 : 1); ++v) {
    const bool repl = up && v == 0;
    for (int c = 0; c < n; ++c) {
      const bool r = repl && c > 0;
      hs[c] = job->hsamp[c];
      vs[c] = job->vsamp[c];
      if (repl) {                                                 // the reference's result: chroma at luma resolution
        hs[c] = c ? 1 : (job->out_hsamp0 > 0 ? job->out_hsamp0 : 1);
        vs[c] = c ? 1 : (job->out_vsamp0 > 0 ? job->out_vsamp0 : 1);
      }
      stride[c] = r ? job->up_wblk : job->wblk[c];
      rows[c] = r ? job->up_hblk : job->hblk[c];
      slot[c] = (up && !repl && c) ? 3 + c : c;
      const int16_t* arr = r ? job->coef_up[c - 1] : job->coef[c];
      if (need_arrays)
        if (int rc = check_array(arr, c, r, who)) return rc;
      if (P) {
        P->coef[slot[c]] = arr;
        P->nblk[slot[c]] = stride[c] * rows[c];
      }
    }
    if (int rc = geometry(job, hs, vs, stride, rows, slot, &D->g[v], who, any_mcu)) return rc;
  }
  D->two = up ? 1 : 0;
  if (info) {
    memset(info, 0, sizeof *info);
    for (int c = 0; c < n; ++c) info->dc_tbl[c] = info->ac_tbl[c] = D->tbl[c];
    info->blocks_in_mcu[0] = D->g[0].bpm;
    info->blocks_in_mcu[1] = up ? D->g[1].bpm : D->g[0].bpm;
  }
  return QS_HIP_OK;
}

// what every prepare leaves for the run calls: the launch chunks that hold a restart job (empty: none), and the workspace
// size the options need.  A workspace that left the registry runs without restart jobs (status 4 for a job that has one)
struct Prepared {
  int njobs;
  uint64_t total;
  std::vector<uint8_t> chunk_restart;
};
QsPrepared<Prepared> g_prepared(4096);

// the descriptors of a batch with their workspace layout; returns the workspace size in *total
int describe_all(qs_hip_job* const* jobs, int njobs, const qs_hip_encode_opts* const* opts, bool need_arrays,
                 std::vector<QsEncJob>& D, std::vector<QsEncPtrs>* P, qs_hip_encode_info* info, uint64_t* total,
                 const char* who) {
  if (!jobs || njobs < 1) return qs_fail(QS_HIP_EINVAL, "%s: %d jobs (at least one)", who, njobs);
  D.assign((size_t)njobs, QsEncJob());
  if (P) P->assign((size_t)njobs, QsEncPtrs());
  Layout L;
  L.take((uint64_t)njobs * sizeof(QsEncJob));                       // the descriptors
  long long wgs = 0, swgs = 0;
  for (int i = 0; i < njobs; ++i) {
    if (int r = describe(jobs[i], &D[i], P ? &(*P)[i] : nullptr, need_arrays, info ? &info[i] : nullptr, Who(who, i).s))
      return r;
    QsEncJob& J = D[i];
    if (i % QS_ENC_CHUNK == 0) wgs = swgs = 0;
    const int nblocks = std::max(J.g[0].nblocks, J.two ? J.g[1].nblocks : 0);
    const qs_hip_encode_opts* o = opts ? opts[i] : nullptr;
    if (o)
      if (int r = qs_enc_check_restart(o->restart_interval, o->restart_in_rows, who, i)) return r;
    uint64_t nint = 1;                                              // restart intervals of the scan, at most
    for (int v = 0; v < (J.two ? 2 : 1); ++v) {
      J.ri[v] = o ? qs_enc_restart(o->restart_interval, o->restart_in_rows, J.g[v]) : 0;
      if (J.ri[v]) nint = std::max<uint64_t>(nint, (uint64_t)ceil_div(J.g[v].mcus, J.ri[v]));
    }
    // (the launch grid of the stuffing kernels does not depend on the options: the run calls do not see them)
    if (int r = qs_enc_scan_layout(L, J, wgs, swgs, nblocks, nint, QS_ENC_MAXBITS, false, who)) return r;
    // every byte stuffed; per interval end a pad byte that may be stuffed, and the two bytes of the marker
    if (info) info[i].max_segment_bytes = 2 * (((uint64_t)nblocks * QS_ENC_MAXBITS + 7) / 8) + 4 * (nint - 1);
  }
  *total = L.total;
  return QS_HIP_OK;
}

// what the whole-file run adds to a run (null: the plain run)
struct FilesRun {
  const qs_hip_encode_frame* frames;
  int optimize;
  qs_hip_huff_tables* d_tables;
  void* d_scratch;
  size_t scratch_bytes;
};

// what the runs and the histogram call share: the chunks' kernel arguments and launches
int enqueue(qs_hip_job* const* jobs, int njobs, const int32_t* d_stop, uint8_t* const* d_out, const size_t* out_capacity,
            uint64_t* d_len, int32_t* d_status, uint32_t* d_counts, void* d_workspace, size_t bytes, void* stream,
            const char* who, const FilesRun* F = nullptr) {
  std::vector<QsEncJob> D;
  std::vector<QsEncPtrs> P;
  uint64_t total = 0;
  if (int r = describe_all(jobs, njobs, nullptr, true, D, &P, nullptr, &total, who)) return r;
  if (!d_counts) {
    if (!d_out || !out_capacity || !d_len || !d_status) return qs_fail(QS_HIP_EINVAL, "%s: null output argument", who);
    for (int i = 0; i < njobs; ++i) {
      if (!d_out[i]) return qs_fail(QS_HIP_EINVAL, "%s: job %d has no output buffer", who, i);
      P[(size_t)i].out = d_out[i];
      P[(size_t)i].cap = out_capacity[i];
    }
  }
  const QsEncScratch FS((uint64_t)njobs);               // (qs_hip_encode_files_scratch_bytes)
  if (F) {
    if (F->frames)
      for (int i = 0; i < njobs; ++i) {
        const qs_hip_encode_frame& f = F->frames[i];
        const int nv = (D[(size_t)i].two && d_stop) ? 2 : 1;        // the variants the device can choose for this job
        for (int v = 0; v < nv; ++v) {
          if ((f.head_bytes[v] && !f.d_head[v]) || (f.mid_bytes[v] && !f.d_mid[v]))
            return qs_fail(QS_HIP_EINVAL, "%s: job %d: variant %d of the frame has a length but no bytes", who, i, v);
          if (!f.d_mid[v] || !f.mid_bytes[v])
            return qs_fail(QS_HIP_EINVAL, "%s: job %d: the frame lacks variant %d (no SOS header), which the job can take",
                           who, i, v);
        }
      }
    if (!workspace_ok(F->d_scratch, F->scratch_bytes, FS.total))
      return qs_fail(QS_HIP_EINVAL, "%s: scratch of %zu bytes (256-byte aligned), %d jobs need %llu", who, F->scratch_bytes,
                     njobs, (unsigned long long)FS.total);
  }
  if (int r = check_workspace(total, d_workspace, bytes, who)) return r;
  // the kernels to launch follow what prepare wrote at this address.  An address not known here (a copy of a prepared
  // workspace, or one that left the registry) runs without restarts, as it always did; the kernels give status 4 to a
  // job whose descriptor has an interval nevertheless, so a lost marker is never silent
  const std::shared_ptr<const Prepared> prep = g_prepared.find(d_workspace);
  if (prep) {
    if (prep->njobs != njobs)
      return qs_fail(QS_HIP_EINVAL, "%s: the workspace was prepared for %d jobs, the call has %d", who, prep->njobs, njobs);
    total = prep->total;
  }
  if (int r = check_workspace(total, d_workspace, bytes, who)) return r;
  if (int r = device_ok()) return r;
  hipStream_t s = static_cast<hipStream_t>(stream);
  for (int j0 = 0; j0 < njobs; j0 += QS_ENC_CHUNK) {
    QsEncArgs a;
    memset(&a, 0, sizeof a);
    a.jobs = static_cast<const QsEncJob*>(d_workspace) + j0;
    a.ws = static_cast<uint8_t*>(d_workspace);
    a.d_stop = d_stop;
    a.d_len = d_len;
    a.d_status = d_status;
    a.d_counts = d_counts;
    a.job0 = j0;
    a.n = std::min(QS_ENC_CHUNK, njobs - j0);
    for (int k = 0; k < a.n; ++k) {
      a.p[k] = P[(size_t)j0 + k];
      a.wg0[k] = D[(size_t)j0 + k].wg0;
      a.swg0[k] = D[(size_t)j0 + k].swg0;
    }
    const QsEncJob& last = D[(size_t)j0 + a.n - 1];
    const bool restart = prep && prep->chunk_restart[(size_t)(j0 / QS_ENC_CHUNK)];
    a.restart = restart ? 1 : 0;
    const int wgs = last.wg0 + last.nwg, swgs = last.swg0 + last.nswg;
    if (!F) {
      qs_launch_encode(a, wgs, swgs, restart, s);
      continue;
    }
    // the whole-file run: [histogram into the scratch, the table kernel,] the coder behind the prefix, the framing
    uint8_t* sc = static_cast<uint8_t*>(F->d_scratch);
    QsHuffArgs h;
    memset(&h, 0, sizeof h);
    h.jobs = a.jobs;
    h.d_stop = d_stop;
    qs_enc_huff_scratch(h, sc, FS);
    h.d_tables = reinterpret_cast<uint8_t*>(F->d_tables);
    h.d_len = d_len;
    h.d_status = d_status;
    h.job0 = j0;
    h.n = a.n;
    h.optimize = F->optimize ? 1 : 0;
    h.framed = F->frames ? 1 : 0;
    for (int k = 0; k < a.n; ++k) {
      QsFramePtrs& f = h.f[k];
      if (F->frames) {
        const qs_hip_encode_frame& src = F->frames[j0 + k];
        for (int v = 0; v < 2; ++v) {
          f.head[v] = src.d_head[v];
          f.mid[v] = src.d_mid[v];
          f.head_bytes[v] = src.d_head[v] ? src.head_bytes[v] : 0;
          f.mid_bytes[v] = src.d_mid[v] ? src.mid_bytes[v] : 0;
          a.fixed[k][v] = f.head_bytes[v] + f.mid_bytes[v];
        }
      }
      f.out = a.p[k].out;
      f.cap = a.p[k].cap;
    }
    if (F->optimize) {
      QsEncArgs hist = a;
      hist.d_counts = reinterpret_cast<uint32_t*>(sc + FS.counts);
      qs_launch_encode(hist, wgs, swgs, restart, s);
      qs_launch_huff_tables(h, s);
      a.codes = h.codes;
      a.tstatus = h.tstatus;
    }
    a.prefix = h.prefix;
    a.tail = F->frames ? 2 : 0;
    qs_launch_encode(a, wgs, swgs, restart, s);
    qs_launch_huff_frame(h, s);
  }
  HIP_TRY(hipGetLastError());
  return QS_HIP_OK;
}

int info_opts(qs_hip_job* const* jobs, int njobs, const qs_hip_encode_opts* const* opts, qs_hip_encode_info* per_job,
              size_t* bytes, const char* who) {
  return guarded([&]() -> int {
    if (!per_job || !bytes) return qs_fail(QS_HIP_EINVAL, "%s: null result", who);
    std::vector<QsEncJob> D;
    uint64_t total = 0;
    if (int r = describe_all(jobs, njobs, opts, false, D, nullptr, per_job, &total, who)) return r;
    *bytes = (size_t)total;
    return QS_HIP_OK;
  });
}

int prepare_opts(qs_hip_job* const* jobs, int njobs, const qs_hip_huff_tables* const* tables,
                 const qs_hip_encode_opts* const* opts, void* d_workspace, size_t bytes, void* stream, const char* who) {
  return guarded([&]() -> int {
    std::vector<QsEncJob> D;
    uint64_t total = 0;
    if (int r = describe_all(jobs, njobs, opts, false, D, nullptr, nullptr, &total, who)) return r;
    for (int i = 0; i < njobs; ++i) {
      const qs_hip_huff_tables* T = tables ? tables[i] : nullptr;
      for (int t = 0; t < 2; ++t) {
        qs_hip_huff_table dc, ac;
        if (T && T->has_dc[t]) dc = T->dc[t]; else standard_table(0, t, &dc);
        if (T && T->has_ac[t]) ac = T->ac[t]; else standard_table(1, t, &ac);
        char what[64];
        snprintf(what, sizeof what, "job %d, DC table %d", i, t);
        if (int r = derive(dc, true, D[(size_t)i].dc[t], 16, who, what)) return r;
        snprintf(what, sizeof what, "job %d, AC table %d", i, t);
        if (int r = derive(ac, false, D[(size_t)i].ac[t], 256, who, what)) return r;
      }
    }
    if (int r = check_workspace(total, d_workspace, bytes, who)) return r;
    if (int r = device_ok()) return r;
    if (int r = upload(d_workspace, D, static_cast<hipStream_t>(stream))) return r;
    Prepared p{njobs, total, std::vector<uint8_t>((size_t)ceil_div(njobs, QS_ENC_CHUNK), 0)};
    for (int i = 0; i < njobs; ++i)
      if (D[(size_t)i].ri[0] || D[(size_t)i].ri[1]) p.chunk_restart[(size_t)(i / QS_ENC_CHUNK)] = 1;
    g_prepared.store(d_workspace, std::move(p));
    return QS_HIP_OK;
  });
}

}  // namespace

int qs_enc_describe(const qs_hip_job* job, QsEncJob* D, QsEncPtrs* P, bool need_arrays, const char* who) {
  return describe(job, D, P, need_arrays, nullptr, who, true);
}

extern "C" int qs_hip_encode_device_batch_info(qs_hip_job* const* jobs, int njobs, qs_hip_encode_info* per_job,
                                               size_t* bytes) {
  return info_opts(jobs, njobs, nullptr, per_job, bytes, "qs_hip_encode_device_batch_info");
}

extern "C" int qs_hip_encode_device_batch_info_opts(qs_hip_job* const* jobs, int njobs,
                                                    const qs_hip_encode_opts* const* opts, qs_hip_encode_info* per_job,
                                                    size_t* bytes) {
  return info_opts(jobs, njobs, opts, per_job, bytes, "qs_hip_encode_device_batch_info_opts");
}

extern "C" int qs_hip_encode_device_batch_prepare(qs_hip_job* const* jobs, int njobs,
                                                  const qs_hip_huff_tables* const* tables, void* d_workspace,
                                                  size_t bytes, void* stream) {
  return prepare_opts(jobs, njobs, tables, nullptr, d_workspace, bytes, stream, "qs_hip_encode_device_batch_prepare");
}

extern "C" int qs_hip_encode_device_batch_prepare_opts(qs_hip_job* const* jobs, int njobs,
                                                       const qs_hip_huff_tables* const* tables,
                                                       const qs_hip_encode_opts* const* opts, void* d_workspace,
                                                       size_t bytes, void* stream) {
  return prepare_opts(jobs, njobs, tables, opts, d_workspace, bytes, stream, "qs_hip_encode_device_batch_prepare_opts");
}

extern "C" int qs_hip_encode_device_batch(qs_hip_job* const* jobs, int njobs, const int32_t* d_stop,
                                          uint8_t* const* d_out, const size_t* out_capacity, uint64_t* d_len,
                                          int32_t* d_status, void* d_workspace, size_t bytes, void* stream) {
  return guarded([&]() -> int {
    return enqueue(jobs, njobs, d_stop, d_out, out_capacity, d_len, d_status, nullptr, d_workspace, bytes, stream,
                   "qs_hip_encode_device_batch");
  });
}

extern "C" int qs_hip_encode_device_batch_histogram(qs_hip_job* const* jobs, int njobs, const int32_t* d_stop,
                                                    uint32_t* d_counts, int32_t* d_status, void* d_workspace,
                                                    size_t bytes, void* stream) {
  return guarded([&]() -> int {
    const char* who = "qs_hip_encode_device_batch_histogram";
    if (!d_counts) return qs_fail(QS_HIP_EINVAL, "%s: null d_counts", who);
    return enqueue(jobs, njobs, d_stop, nullptr, nullptr, nullptr, d_status, d_counts, d_workspace, bytes, stream, who);
  });
}

extern "C" size_t qs_hip_encode_files_scratch_bytes(int njobs) { return (size_t)QsEncScratch((uint64_t)std::max(njobs, 0)).total; }

extern "C" int qs_hip_encode_device_batch_files(qs_hip_job* const* jobs, int njobs, const qs_hip_encode_frame* frames,
                                                int optimize, const int32_t* d_stop, uint8_t* const* d_out,
                                                const size_t* out_capacity, uint64_t* d_len, int32_t* d_status,
                                                qs_hip_huff_tables* d_tables, void* d_scratch, size_t scratch_bytes,
                                                void* d_workspace, size_t bytes, void* stream) {
  return guarded([&]() -> int {
    const FilesRun F{frames, optimize, d_tables, d_scratch, scratch_bytes};
    return enqueue(jobs, njobs, d_stop, d_out, out_capacity, d_len, d_status, nullptr, d_workspace, bytes, stream,
                   "qs_hip_encode_device_batch_files", &F);
  });
}

extern "C" int qs_hip_huff_optimal_device(const uint32_t* d_counts, int ntables, qs_hip_huff_table* d_tables,
                                          int32_t* d_status, void* stream) {
  const char* who = "qs_hip_huff_optimal_device";
  if (!d_counts || !d_tables || !d_status || ntables < 1) return qs_fail(QS_HIP_EINVAL, "%s: null argument or no table", who);
  if (int r = device_ok()) return r;
  qs_launch_huff_optimal(d_counts, ntables, reinterpret_cast<uint8_t*>(d_tables), d_status, static_cast<hipStream_t>(stream));
  HIP_TRY(hipGetLastError());
  return QS_HIP_OK;
}

extern "C" int qs_hip_huff_standard(int is_ac, int tbl, uint8_t bits[17], uint8_t huffval[256]) {
  if (tbl < 0 || tbl > 1 || !bits || !huffval) return qs_fail(QS_HIP_EINVAL, "qs_hip_huff_standard: table 0 or 1");
  qs_hip_huff_table t;
  standard_table(is_ac != 0, tbl, &t);
  memcpy(bits, t.bits, 17);
  memcpy(huffval, t.huffval, 256);
  return QS_HIP_OK;
}

// jpeg_gen_optimal_table of jchuff.c (JPEG Annex K.2): Huffman's procedure with the reserved pseudo-symbol 256 and code
// lengths cut back to 16 (figure K.3) give the number of codes of each length.  The symbols are listed as libjpeg 9d
// lists them: by falling count, equal counts by rising value -- so a more frequent symbol never has the longer code,
// also where the cut-back split a length (the 9c and earlier order, by length then value, differs in the DHT bytes)
extern "C" int qs_hip_huff_optimal(const uint32_t freq_in[257], uint8_t bits_out[17], uint8_t huffval[256]) {
  if (!freq_in || !bits_out || !huffval) return qs_fail(QS_HIP_EINVAL, "qs_hip_huff_optimal: null argument");
  return guarded([&]() -> int {
    // the procedure of csrc/qs_huff.h, the table kernel's, in its host form
    static thread_local QsHuffShared S;
    if (qs_huff_wave(freq_in, S) != QS_HF_OK) return qs_fail(QS_HIP_EINVAL, "qs_hip_huff_optimal: code length overflow");
    memcpy(bits_out, S.outbits, 17);
    memcpy(huffval, S.huffval, 256);
    return QS_HIP_OK;
  });
}
