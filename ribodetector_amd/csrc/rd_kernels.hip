// rd_kernels.hip - CDNA4 (gfx950) kernels + C ABI of the RiboDetector BiLSTM inference path.
//
// Reference path being replaced (paths relative to /root/reference/ribodetector):
//   data_loader/seq_encoder.py:11-18,126-127   one-hot nucleotide encoder
//   detect.py:666-726                          collate: truncate to max_len, one-hot, pack_sequence
//   model/model.py:32-37,114-119               forward1: BiLSTM, last-timestep gather, Linear(256->2)
//   detect.py:288,481                          argmax
//   detect.py:616-663                          paired-end label fusion
//
// Structural facts used (verified by tests against the reference's own outputs):
//   * forward1 gathers timestep len-1. There the reverse LSTM has made exactly ONE step from the zero state,
//     so its contribution to the logits is a 5-entry table keyed by the last base (rev_lut).
//   * the input is one-hot/zero, so W_ih x + b_ih + b_hh is a 5-row table (in_lut) - a gather, not a GEMM.
//   => the only dense work is the forward recurrence h[B,128] . W_hh^T[128,512] per timestep.
//
// Kernel inventory (DESIGN.md §3 has the roofline of each)
//   rd_prep_kernel, rd_revtab_kernel   weight pre-packing (once per model); reverse-half table of the padded semantics
//   rd_steps_kernel, rd_bucket_scan/scatter_kernel   steps per read + length bucketing for rd_classify (longest first)
//   rd_len_hist/scan/scatter_kernel    stable counting sort = pack_sequence's sort, for rd_pack_plan
//   rd_lstm_mfma_f16x3_t32_kernel      DEFAULT recurrence: split-precision f16 MFMA 32x32x16, weights resident in AGPRs,
//                                      hand-interleaved gate math; fused encoder + FC + argmax epilogue
//   rd_lstm_mfma_f32_kernel            exact-fp32 MFMA recurrence (A/B reference for the split-precision kernels)
//   rd_lstm_simple_kernel              plain-FMA cross-check of the same function
//   rd_refine_kernel                   float64 re-evaluation of the reads whose margin is inside the fp32 noise band
//   rd_encode_* / rd_pack_onehot       standalone encoder kernels (reference tensor layouts), HBM-bound
//   rd_pair_fuse_kernel, rd_count_kernel
//   rd_gz_*                            records of one label -> gzip (BGZF) members on the device (rd_deflate.hpp)
//   rd_group_* / rd_gz_compress_grouped the records partitioned by key: a run of text or of members per key (rd_group_pack.hpp)
//   rd_fq_* / rd_fa_*                  FASTQ records framed, FASTA batches re-written and indexed in HBM (rd_fastq_index.hpp, rd_fasta_index.hpp)
//   rd_report_*                        per-read report lines (id, label, probabilities) of a chunk (rd_report.hpp)
//   rd_pair_*                          the mates of an interleaved chunk: pair table, mates' sequence tables, mate check (rd_pairs.hpp)
//   rd_summary_*                       the QC counters of a run, added up chunk by chunk (rd_summary.hpp)
//   rd_bam_find_*, rd_bam_count        a record start behind an offset of inflated BAM bytes, the records of a share (rd_bam_shard.hpp)
//   rd_bam_tag_find, rd_bam_group_*    the optional fields of raw BAM records, and the counters per read group (rd_bam_tags.hpp)
//   rd_bam_tag_splice                  the listed tags as text behind the read names of the FASTQ text (rd_bam_tagtext.hpp)
//   rd_bam_encode                      the records of a FASTQ / FASTA chunk as unaligned BAM records: --ubam_output (rd_bam_encode.hpp)
//   rd_float_text                      float32 values as their exact %g text; the f / B:f values of rd_bam_tag_splice_ex (rd_float_text.hpp)
//   rd_float_parse                     the text of float values as the nearest float32; the f / B:f values of rd_bam_encode_ex (rd_float_parse.hpp)
//   rd_window_*                        reads longer than max_len as several windows: the window table and the fusion of its logits (rd_windows.hpp)
//   rd_region_*                        the rRNA stretches of reads classified over windows, as text lines (rd_regions.hpp)
#include <stdlib.h>
#include "rd_common.hpp"
#include "rd_prep.hpp"
#include "rd_recurrence.hpp"
#include "rd_sort.hpp"
#include "rd_lstm_f32.hpp"
#include "rd_lstm_t32.hpp"
#include "rd_refine.hpp"
#include "rd_encode.hpp"
#include "rd_scan.hpp"
#include "rd_deflate.hpp"
#include "rd_inflate_dev.hpp"
#include "rd_inflate_stream.hpp"
#include "rd_fastq_index.hpp"
#include "rd_fasta_index.hpp"
#include "rd_bam_index.hpp"
#include "rd_bam_shard.hpp"
#include "rd_bam_raw.hpp"
#include "rd_report.hpp"
#include "rd_pairs.hpp"
#include "rd_summary.hpp"
#include "rd_bam_tags.hpp"
#include "rd_bam_tagtext.hpp"
#include "rd_bam_encode.hpp"
#include "rd_windows.hpp"
#include "rd_regions.hpp"
#include "rd_group_pack.hpp"

// ================================================================================================
// C ABI
// ================================================================================================
extern "C" {

const char *rd_last_error(void) { return g_err; }
const char *rd_version(void) { return "ribodetector_amd 0.1.0 (gfx950)"; }

// host-side, before any device call: the weights the kernels can represent (include/ribodetector_amd.h)
int rd_weights_check(const rd_weights *w) {
    if (!w) RD_FAIL(RD_E_INVALID, "rd_weights_check: null argument");
    if (w->input_size != 4 || w->hidden_size != HID || w->num_classes != 2)
        RD_FAIL(RD_E_UNSUPPORTED, "rd_model_create: kernels cover input_size=4, hidden_size=128, num_classes=2 (got %d,%d,%d)",
                w->input_size, w->hidden_size, w->num_classes);
    const float *src[10] = {w->w_ih, w->w_hh, w->b_ih, w->b_hh, w->w_ih_r, w->w_hh_r, w->b_ih_r, w->b_hh_r, w->w_out, w->b_out};
    const int offs[11] = {OFF_WIH, OFF_WHH, OFF_BIH, OFF_BHH, OFF_WIHR, OFF_WHHR, OFF_BIHR, OFF_BHHR, OFF_WOUT, OFF_BOUT, RAW_FLOATS};
    static const char *const names[10] = {"rnn.weight_ih_l0", "rnn.weight_hh_l0", "rnn.bias_ih_l0", "rnn.bias_hh_l0", "rnn.weight_ih_l0_reverse",
                                          "rnn.weight_hh_l0_reverse", "rnn.bias_ih_l0_reverse", "rnn.bias_hh_l0_reverse", "out.weight", "out.bias"};
    for (int i = 0; i < 10; ++i)
        if (!src[i]) RD_FAIL(RD_E_INVALID, "rd_model_create: weight pointer %d is null", i);
    for (int i = 0; i < 10; ++i) {
        const int n = offs[i + 1] - offs[i];
        for (int k = 0; k < n; ++k)
            if (!(fabsf(src[i][k]) <= 3.402823466e38f))
                RD_FAIL(RD_E_INVALID, "rd_model_create: %s holds a non-finite value (%g at element %d)", names[i], (double)src[i][k], k);
    }
    float mx = 0.0f;
    for (int k = 0; k < G4 * HID; ++k) mx = fmaxf(mx, fabsf(w->w_hh[k]));
    if (mx >= 65504.0f / 16.0f)
        RD_FAIL(RD_E_UNSUPPORTED, "rd_model_create: max |rnn.weight_hh_l0| = %g is not below 65504/16 = 4094: the split-precision kernel stores "
                                  "16 w in fp16", (double)mx);
    return RD_OK;
}

int rd_model_create(const rd_weights *w, int device, rd_model **out) {
    if (!w || !out) RD_FAIL(RD_E_INVALID, "rd_model_create: null argument");
    if (const int rc = rd_weights_check(w)) return rc;
    const float *src[10] = {w->w_ih, w->w_hh, w->b_ih, w->b_hh, w->w_ih_r, w->w_hh_r, w->b_ih_r, w->b_hh_r, w->w_out, w->b_out};
    const int offs[11] = {OFF_WIH, OFF_WHH, OFF_BIH, OFF_BHH, OFF_WIHR, OFF_WHHR, OFF_BIHR, OFF_BHHR, OFF_WOUT, OFF_BOUT, RAW_FLOATS};
    RD_HIP(hipSetDevice(device));
    rd_model *m = new rd_model();
    memset(m, 0, sizeof(*m));
    m->device = device;
    m->variant = RD_VARIANT_MFMA_F16X3_T32;
    m->refine_thresh = RD_REFINE_DEFAULT;
    m->prefix_k = 0;
    float *host = new float[RAW_FLOATS];
    for (int i = 0; i < 10; ++i) memcpy(host + offs[i], src[i], sizeof(float) * (size_t)(offs[i + 1] - offs[i]));
    hipError_t e = hipSuccess;
    auto A = [&](void **p, size_t bytes) { if (e == hipSuccess) e = hipMalloc(p, bytes); };
    A((void **)&m->d.raw, sizeof(float) * RAW_FLOATS);
    A((void **)&m->d.wpack32, sizeof(float) * 4 * 8 * 32 * 64);
    A((void **)&m->d.wt_hh, sizeof(float) * HID * G4);
    A((void **)&m->d.wpack16b, sizeof(uint16_t) * 4 * 2 * 4 * 8 * 64 * 8);
    A((void **)&m->d.in_lut, sizeof(float) * 5 * G4);
    A((void **)&m->d.lut_t32, sizeof(float) * 4 * 2 * 4 * 4 * 6 * 4);
    A((void **)&m->d.rev_lut, sizeof(float) * 10);
    A((void **)&m->d.rev_tab, sizeof(float) * (size_t)MAX_LEN_LIMIT * 10);
    A((void **)&m->d.w_out, sizeof(float) * 512);
    A((void **)&m->d.b_out, sizeof(float) * 2);
    A((void **)&m->d.zero_row, PFX_ROW);
    if (e == hipSuccess) e = hipMemset(m->d.zero_row, 0, PFX_ROW);
    if (e == hipSuccess) e = hipMemcpy(m->d.raw, host, sizeof(float) * RAW_FLOATS, hipMemcpyHostToDevice);
    delete[] host;
    if (e == hipSuccess) {
        hipLaunchKernelGGL(rd_prep_kernel, dim3(64), dim3(256), 0, 0, m->d);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) {
        snprintf(g_err, sizeof(g_err), "rd_model_create: %s", hipGetErrorString(e));
        rd_model_destroy(m);
        return RD_E_HIP;
    }
    m->ptab = m->d.zero_row;
    *out = m;
    return RD_OK;
}

void rd_model_destroy(rd_model *m) {
    if (!m) return;
    hipSetDevice(m->device);
    if (m->side) { hipStreamSynchronize(m->side); hipStreamDestroy(m->side); }
    if (m->ev_fork) hipEventDestroy(m->ev_fork);
    for (int x = 0; x < 2; ++x) {
        if (m->ev_join[x]) hipEventDestroy(m->ev_join[x]);
        if (m->q_e[x]) hipFree(m->q_e[x]);
        if (m->q_count[x]) hipFree(m->q_count[x]);
    }
    hipFree(m->d.raw); hipFree(m->d.wpack32); hipFree(m->d.wt_hh); hipFree(m->d.in_lut);
    hipFree(m->d.rev_lut); hipFree(m->d.rev_tab); hipFree(m->d.w_out); hipFree(m->d.b_out);
    if (m->d.wpack16b) hipFree(m->d.wpack16b);
    if (m->d.lut_t32) hipFree(m->d.lut_t32);
    if (m->d.zero_row) hipFree(m->d.zero_row);
    for (int i = 0; i < 2 * 512; ++i)
        if (m->prof_ev[i]) hipEventDestroy(m->prof_ev[i]);
    delete m;
}

// Product build: the three kernels that compute the function (AUTO = the split-precision MFMA kernel). The A/B and diagnostic
// instantiations of the exact-fp32 kernel (ids 10-23; several compute WRONG results by design: gate math or MFMAs removed) exist
// only in the -DRD_DIAG build (librd_hip_diag.so, tools/), never in librd_hip.so. (The experiment copy of the default kernel of
// rounds 1-3, rd_lstm_t32_diag.hpp, was removed in round 4: ONE body of that kernel; its results are in profiles/ and DESIGN.md §8.)
static bool rd_variant_known(int v) {
    if (v == RD_VARIANT_MFMA_F32 || v == RD_VARIANT_SIMPLE || v == RD_VARIANT_MFMA_F16X3_T32) return true;
#ifdef RD_DIAG
    switch (v) {
    case 10: case 11: case 12: case 13: case 20: case 21: case 22: case 23: return true;
    default: break;
    }
#endif
    return false;
}

int rd_variant_available(int variant) { return (variant == RD_VARIANT_AUTO || rd_variant_known(variant)) ? 1 : 0; }

int rd_set_variant(rd_model *m, int variant) {
    if (!m) RD_FAIL(RD_E_INVALID, "rd_set_variant: null model");
    if (variant == RD_VARIANT_AUTO) variant = RD_VARIANT_MFMA_F16X3_T32;
    if (!rd_variant_known(variant))
        RD_FAIL(RD_E_UNSUPPORTED, "rd_set_variant: variant %d not available in this build (product build: 0 auto, 1 mfma_f32, 2 simple, 4 mfma_f16x3_t32)", variant);
    m->variant = variant;
    return RD_OK;
}

int rd_set_semantics(rd_model *m, int semantics) {
    if (!m) RD_FAIL(RD_E_INVALID, "rd_set_semantics: null model");
    if (semantics != RD_SEM_PACKED && semantics != RD_SEM_PADDED) RD_FAIL(RD_E_INVALID, "rd_set_semantics: unknown semantics %d", semantics);
    m->semantics = semantics;
    return RD_OK;
}

int rd_set_refine(rd_model *m, float thresh) {
    if (!m) RD_FAIL(RD_E_INVALID, "rd_set_refine: null model");
    if (!(thresh >= 0.0f) || thresh > 1.0f) RD_FAIL(RD_E_INVALID, "rd_set_refine: threshold %g out of range [0, 1]", (double)thresh);
    m->refine_thresh = thresh;
    return RD_OK;
}

constexpr uint32_t RD_REFINE_QCAP = 8192;   // candidates a queue holds (an overflow is caught by the second tier of rd_async_flush)

static RefineQueue rd_queue(const rd_model *m, int x) { return RefineQueue{(RefineEntry *)m->q_e[x], m->q_count[x], RD_REFINE_QCAP}; }

// evaluate the candidates waiting in queue x on the model's stream, beside whatever `st` does next
static int rd_async_flush(rd_model *m, hipStream_t st, int x) {
    RD_HIP(hipEventRecord(m->ev_fork, st));
    RD_HIP(hipStreamWaitEvent(m->side, m->ev_fork, 0));
    hipLaunchKernelGGL(rd_refine_flush_kernel, dim3(REFINE_FLUSH_WGS), dim3(1024), 0, m->side, m->d, rd_queue(m, x));
    for (int k = 0; k < m->q_npend[x]; ++k) {   // second tier: launches that return at once unless the queue overflowed
        const auto &pd = m->q_pend[x][k];
        ReadBatch rb{(const uint8_t *)pd.p[0], (const int64_t *)pd.p[1], (const int32_t *)pd.p[2], nullptr, nullptr, pd.n, pd.max_len, pd.sem,
                     m->d.rev_tab, nullptr, nullptr, 0, RefineQueue{nullptr, nullptr, 0}, 0.0f};
        int64_t nb = (pd.n + REFINE_SLICE - 1) / REFINE_SLICE;
        if (nb > 16) nb = 16;   // the workgroups walk the slices (gate closed: sixteen workgroups look at it and leave)
        hipLaunchKernelGGL(rd_refine_kernel, dim3((unsigned)nb), dim3(1024), 0, m->side, m->d, rb, (const float2 *)nullptr, pd.thresh,
                           (float *)pd.p[3], (uint8_t *)pd.p[4], rd_queue(m, x), (const uint32_t *)m->q_count[x]);
    }
    RD_HIP(hipGetLastError());
    RD_HIP(hipMemsetAsync(m->q_count[x], 0, sizeof(uint32_t), m->side));
    RD_HIP(hipEventRecord(m->ev_join[x], m->side));
    m->q_flushing[x] = 1;
    m->q_wait[x] = 1;
    return RD_OK;
}

// queue x is about to take the candidates of a call issued on `st`: its last flush (and the reset of its counter) comes first. The
// stream that joined that flush has waited already; a rd_sync_results on ANOTHER stream (a caller's post-processing stream) has not
// ordered `st` behind it - the flush is long finished by then (it takes 0.3 ms, a recurrence launch tens), this makes it formal.
static int rd_async_acquire(rd_model *m, hipStream_t st, int x) {
    if (m->q_wait[x]) {
        RD_HIP(hipStreamWaitEvent(st, m->ev_join[x], 0));
        m->q_wait[x] = 0;
    }
    return RD_OK;
}

// everything issued on `st` from here on sees the results of the calls whose candidates were in queue x
static int rd_async_join(rd_model *m, hipStream_t st, int x) {
    if (m->q_flushing[x]) {
        RD_HIP(hipStreamWaitEvent(st, m->ev_join[x], 0));
        m->q_flushing[x] = 0;
        m->q_npend[x] = 0;
    }
    return RD_OK;
}

int rd_sync_results(rd_model *m, void *stream) {
    if (!m) RD_FAIL(RD_E_INVALID, "rd_sync_results: null model");
    if (!m->refine_async) return RD_OK;
    hipStream_t st = (hipStream_t)stream;
    int rc = RD_OK;
    if (m->q_calls > 0) {
        rc = rd_async_flush(m, st, m->q_cur);
        if (rc) return rc;
        m->q_cur ^= 1;   // calls issued from here on (on whatever stream) record into the other queue while this one is evaluated
        m->q_calls = 0;
    }
    for (int x = 0; x < 2 && !rc; ++x) rc = rd_async_join(m, st, x);
    return rc;
}

int rd_set_refine_async(rd_model *m, int calls) {
    if (!m) RD_FAIL(RD_E_INVALID, "rd_set_refine_async: null model");
    if (calls < 0 || calls > 16) RD_FAIL(RD_E_INVALID, "rd_set_refine_async: calls per group %d out of range [0, 16]", calls);
    if (m->q_calls || m->q_flushing[0] || m->q_flushing[1])
        RD_FAIL(RD_E_INVALID, "rd_set_refine_async: calls are pending - rd_sync_results first");
    if (calls && !m->side) {
        RD_HIP(hipSetDevice(m->device));
        // highest priority: when a CU becomes free its workgroups go first - a workgroup of the float64 pass needs a whole CU (1,024
        // threads), and so does every workgroup of the recurrence kernel that the pass is meant to run beside
        int lo = 0, hi = 0;
        RD_HIP(hipDeviceGetStreamPriorityRange(&lo, &hi));
        const char *pr = getenv("RD_REFINE_STREAM_PRIORITY");   // (A/B knob: "low" / "normal"; default high)
        const int prio = pr && !strcmp(pr, "low") ? lo : pr && !strcmp(pr, "normal") ? (lo + hi) / 2 : hi;
        RD_HIP(hipStreamCreateWithPriority(&m->side, hipStreamNonBlocking, prio));
        RD_HIP(hipEventCreateWithFlags(&m->ev_fork, hipEventDisableTiming));
        for (int x = 0; x < 2; ++x) {
            RD_HIP(hipEventCreateWithFlags(&m->ev_join[x], hipEventDisableTiming));
            RD_HIP(hipMalloc(&m->q_e[x], sizeof(RefineEntry) * RD_REFINE_QCAP));
            RD_HIP(hipMalloc((void **)&m->q_count[x], sizeof(uint32_t)));
            RD_HIP(hipMemset(m->q_count[x], 0, sizeof(uint32_t)));
        }
    }
    m->refine_async = calls;
    return RD_OK;
}

static int rd_refine_launch(rd_model *m, const ReadBatch &rb, float *logits, uint8_t *labels, const float *mate_logits, float thresh,
                            hipStream_t st) {
    const int64_t nb = (rb.n + REFINE_SLICE - 1) / REFINE_SLICE;
    hipLaunchKernelGGL(rd_refine_kernel, dim3((unsigned)nb), dim3(1024), 0, st, m->d, rb, (const float2 *)mate_logits, thresh, logits, labels,
                       RefineQueue{nullptr, nullptr, 0}, (const uint32_t *)nullptr);
    RD_HIP(hipGetLastError());
    return RD_OK;
}

int rd_refine(const rd_model *cm, const uint8_t *arena, const int64_t *seq_off, const int32_t *seq_len, int64_t n, int32_t max_len,
              float *logits, uint8_t *labels, const float *mate_logits, float thresh, void *stream) {
    rd_model *m = const_cast<rd_model *>(cm);
    if (!m || !logits) RD_FAIL(RD_E_INVALID, "rd_refine: null model or logits");
    if (n < 0 || n > 0x7fffffffLL) RD_FAIL(RD_E_INVALID, "rd_refine: n=%lld out of range", (long long)n);
    if (max_len < 1 || max_len > MAX_LEN_LIMIT) RD_FAIL(RD_E_INVALID, "rd_refine: max_len=%d out of range [1,%d]", max_len, MAX_LEN_LIMIT);
    if (!(thresh <= 1.0f)) RD_FAIL(RD_E_INVALID, "rd_refine: threshold %g out of range", (double)thresh);
    if (thresh <= 0.0f) thresh = m->refine_thresh;   // the model's band
    if (n == 0 || thresh <= 0.0f) return RD_OK;
    if (!arena || !seq_off || !seq_len) RD_FAIL(RD_E_INVALID, "rd_refine: null input pointer");
    hipStream_t st = (hipStream_t)stream;
    if (m->refine_async) { int rc0 = rd_sync_results(m, stream); if (rc0) return rc0; }   // the logits it reads may have candidates waiting
    // padded semantics: the reverse-half table is built by rd_classify for ITS max_len, on ITS stream. Rebuilding it here - typically
    // on a side stream, while a recurrence kernel of the main stream reads it - would be a data race (advisor finding, round 2), so
    // the pass refuses a max_len the table was not built for: it re-evaluates reads of an earlier rd_classify call by definition.
    if (m->semantics == RD_SEM_PADDED && m->rev_tab_len != max_len)
        RD_FAIL(RD_E_INVALID, "rd_refine: padded semantics needs a preceding rd_classify with the same max_len (table built for %d, got %d)",
                m->rev_tab_len, max_len);
    ReadBatch rb{arena, seq_off, seq_len, nullptr, nullptr, n, max_len, m->semantics, m->d.rev_tab, nullptr, nullptr, 0,
                 RefineQueue{nullptr, nullptr, 0}, 0.0f};
    return rd_refine_launch(m, rb, logits, labels, mate_logits, thresh, st);
}

size_t rd_prefix_table_bytes(int32_t k) {
    if (k < RD_PREFIX_K_MIN || k > RD_PREFIX_K_MAX) return 0;
    return (((size_t)1 << (2 * k)) + 1) * PFX_ROW;
}

size_t rd_prefix_scratch_bytes(int32_t k) {
    if (k < RD_PREFIX_K_MIN || k > RD_PREFIX_K_MAX) return 0;
    return ((size_t)1 << (2 * (k - 1))) * PFX_ROW;
}

int rd_prefix_k(const rd_model *m) { return m ? m->prefix_k : 0; }

int rd_set_prefix_table(rd_model *m, int32_t k, void *table, size_t table_bytes, void *scratch, size_t scratch_bytes, void *stream) {
    if (!m) RD_FAIL(RD_E_INVALID, "rd_set_prefix_table: null model");
    if (k == 0) {
        m->prefix_k = 0;
        m->ptab = m->d.zero_row;
        m->ptab_variant = 0;
        return RD_OK;
    }
    if (m->variant != RD_VARIANT_MFMA_F16X3_T32 && m->variant != RD_VARIANT_MFMA_F32)
        RD_FAIL(RD_E_UNSUPPORTED, "rd_set_prefix_table: kernel variant %d has no prefix-state table (mfma_f16x3_t32 and mfma_f32 do)", m->variant);
    const size_t need = rd_prefix_table_bytes(k), need_s = rd_prefix_scratch_bytes(k);
    if (!need) RD_FAIL(RD_E_INVALID, "rd_set_prefix_table: k=%d out of range [%d,%d] (or 0 = none)", k, RD_PREFIX_K_MIN, RD_PREFIX_K_MAX);
    if (!table || ((uintptr_t)table & 255) || !scratch || ((uintptr_t)scratch & 255))
        RD_FAIL(RD_E_INVALID, "rd_set_prefix_table: table and scratch must be 256-byte aligned device pointers");
    if (table_bytes < need) RD_FAIL(RD_E_WORKSPACE, "rd_set_prefix_table: table too small for k=%d: %zu < %zu", k, table_bytes, need);
    if (scratch_bytes < need_s) RD_FAIL(RD_E_WORKSPACE, "rd_set_prefix_table: scratch too small for k=%d: %zu < %zu", k, scratch_bytes, need_s);
    hipStream_t st = (hipStream_t)stream;
    uint8_t *tab = (uint8_t *)table, *scr = (uint8_t *)scratch;
    // level j (the states after every j-base prefix) from level j-1, one step per launch; the levels alternate between the table
    // and the scratch so that level k lands in the table (level k-1, a part of its size, is the largest one in the scratch)
    const uint8_t *prev = m->d.zero_row;
    for (int j = 1; j <= k; ++j) {
        uint8_t *dst = ((k - j) & 1) ? scr : tab;
        const int64_t rows = (int64_t)1 << (2 * j);
        ReadBatch rb{nullptr, nullptr, nullptr, nullptr, nullptr, rows, 1, RD_SEM_PACKED, nullptr, prev, nullptr, j,
                     RefineQueue{nullptr, nullptr, 0}, 0.0f};
        const dim3 grid((unsigned)((rows + 63) / 64)), blk(256);
        if (m->variant == RD_VARIANT_MFMA_F32)   // the rows are the state of the kernel that builds them: each kernel its own table
            hipLaunchKernelGGL((rd_lstm_mfma_f32_kernel<2, 0, 0, true>), grid, blk, 0, st, m->d, rb, (float *)dst, (uint8_t *)nullptr);
        else
            hipLaunchKernelGGL(rd_lstm_mfma_f16x3_t32_kernel<true>, grid, blk, 0, st, m->d, rb, (float *)dst, (uint8_t *)nullptr);
        prev = dst;
    }
    RD_HIP(hipGetLastError());
    RD_HIP(hipMemsetAsync(tab + ((size_t)1 << (2 * k)) * PFX_ROW, 0, PFX_ROW, st));   // the zero row: reads that cannot use a prefix row
    RD_HIP(hipStreamSynchronize(st));
    m->prefix_k = k;
    m->ptab = tab;
    m->ptab_variant = m->variant;
    return RD_OK;
}

size_t rd_classify_workspace_bytes(int64_t n, int32_t max_len) {
    if (n < 0 || max_len < 1) return 0;
    return sort_ws(nullptr, n, max_len).total;
}

int rd_profile_enable(rd_model *m, int enable) {
    if (!m) RD_FAIL(RD_E_INVALID, "rd_profile_enable: null model");
    m->prof_enabled = enable;
    m->prof_count = 0;
    m->prof_ms_accum = 0;
    m->prof_launches_accum = 0;
    return RD_OK;
}

static int rd_profile_drain(rd_model *m) {
    for (int i = 0; i < m->prof_count; ++i) {
        float ms = 0;
        RD_HIP(hipEventSynchronize(m->prof_ev[2 * i + 1]));
        RD_HIP(hipEventElapsedTime(&ms, m->prof_ev[2 * i], m->prof_ev[2 * i + 1]));
        m->prof_ms_accum += ms;
        m->prof_launches_accum += 1;
    }
    m->prof_count = 0;
    return RD_OK;
}

int rd_profile_read(rd_model *m, int64_t *launches, double *total_ms) {
    if (!m) RD_FAIL(RD_E_INVALID, "rd_profile_read: null model");
    int rc = rd_profile_drain(m);
    if (rc) return rc;
    if (launches) *launches = m->prof_launches_accum;
    if (total_ms) *total_ms = m->prof_ms_accum;
    return RD_OK;
}

int rd_classify(const rd_model *cm, const uint8_t *arena, const int64_t *seq_off, const int32_t *seq_len, int64_t n,
                int32_t max_len, float *logits, uint8_t *labels, void *workspace, size_t workspace_bytes, void *stream) {
    rd_model *m = const_cast<rd_model *>(cm);
    if (!m || !logits) RD_FAIL(RD_E_INVALID, "rd_classify: null model or logits");
    if (n < 0 || n > 0x7fffffffLL) RD_FAIL(RD_E_INVALID, "rd_classify: n=%lld out of range", (long long)n);
    if (max_len < 1 || max_len > MAX_LEN_LIMIT) RD_FAIL(RD_E_INVALID, "rd_classify: max_len=%d out of range [1,%d]", max_len, MAX_LEN_LIMIT);
    if (n == 0) return RD_OK;
    if (!arena || !seq_off || !seq_len || !workspace) RD_FAIL(RD_E_INVALID, "rd_classify: null input pointer");
    hipStream_t st = (hipStream_t)stream;
    const size_t need = sort_ws(nullptr, n, max_len).total;
    if (workspace_bytes < need) RD_FAIL(RD_E_WORKSPACE, "workspace too small: %zu < %zu", workspace_bytes, need);
    // deferred float64 pass (rd_set_refine_async): not inside a stream capture (a captured call stays self-contained)
    bool deferred = false;
    int join_after_launch = -1;
    if (m->refine_async && m->refine_thresh > 0.0f) {
        hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
        (void)hipStreamIsCapturing(st, &cap);
        deferred = cap == hipStreamCaptureStatusNone;
    }
    if (deferred) {
        // a call that touches a buffer of a call whose candidates still wait (or are being evaluated) gets the finished results first
        bool clash = false;
        for (int x = 0; x < 2 && !clash; ++x)
            for (int k = 0; k < m->q_npend[x] && !clash; ++k) {
                const auto &pd = m->q_pend[x][k];
                const char *lo = (const char *)pd.p[3], *la = (const char *)pd.p[4];
                clash = (m->semantics == RD_SEM_PADDED && pd.max_len != max_len) ||   // (the padded table would be rebuilt under the flush)
                        arena == pd.p[0] || seq_off == pd.p[1] || seq_len == pd.p[2] ||
                        ((const char *)logits < lo + 8 * pd.n && lo < (const char *)logits + 8 * n) ||
                        (labels && la && (const char *)labels < la + pd.n && la < (const char *)labels + n);
            }
        if (clash) { int rc0 = rd_sync_results(m, stream); if (rc0) return rc0; }
        if (m->q_calls >= m->refine_async) {   // the group is complete: its candidates are evaluated beside THIS call's recurrence
            const int old = m->q_cur;
            int rc0 = rd_async_flush(m, st, old);
            if (rc0) return rc0;
            m->q_cur ^= 1;
            m->q_calls = 0;
            rc0 = rd_async_join(m, st, m->q_cur);   // the other queue's flush was issued a whole group ago
            if (rc0) return rc0;
            join_after_launch = old;
        }
        int rc1 = rd_async_acquire(m, st, m->q_cur);
        if (rc1) return rc1;
    }
    if (m->semantics == RD_SEM_PADDED && m->rev_tab_len != max_len) {   // (after the block above: candidates of another max_len that
        hipLaunchKernelGGL(rd_revtab_kernel, dim3(1), dim3(512), 0, st, m->d, max_len);   // still waited have been evaluated by now)
        m->rev_tab_len = max_len;
    }
    int32_t *steps = nullptr, *order = nullptr, *pfx = nullptr;
    const int pk = m->variant == m->ptab_variant ? m->prefix_k : 0;      // the rows hold the state of the kernel that built them
    int rc = run_steps_and_buckets(arena, seq_off, seq_len, n, max_len, m->semantics, workspace, workspace_bytes, steps, order, pk, pfx, st);
    if (rc) return rc;
    ReadBatch rb{arena, seq_off, seq_len, steps, order, n, max_len, m->semantics, m->d.rev_tab, pk > 0 ? m->ptab : m->d.zero_row, pfx, pk,
                 deferred ? rd_queue(m, m->q_cur) : RefineQueue{nullptr, nullptr, 0}, m->refine_thresh};
    hipEvent_t *ev = nullptr;
    if (m->prof_enabled) {
        if (m->prof_count == 512) { rc = rd_profile_drain(m); if (rc) return rc; }
        ev = &m->prof_ev[2 * m->prof_count];
        for (int i = 0; i < 2; ++i)
            if (!ev[i]) RD_HIP(hipEventCreate(&ev[i]));
        RD_HIP(hipEventRecord(ev[0], st));
    }
    if (m->variant == RD_VARIANT_SIMPLE) {
        const int64_t nwg = (n + SB - 1) / SB;
        hipLaunchKernelGGL(rd_lstm_simple_kernel, dim3((unsigned)nwg), dim3(512), 0, st, m->d, rb, logits, labels);
    } else {
        const int64_t nwg = (n + BT - 1) / BT;
        const dim3 grid((unsigned)nwg), blk(256);
        switch (m->variant) {
        case RD_VARIANT_MFMA_F16X3_T32: hipLaunchKernelGGL(rd_lstm_mfma_f16x3_t32_kernel<false>, grid, blk, 0, st, m->d, rb, logits, labels); break;
        case RD_VARIANT_MFMA_F32: hipLaunchKernelGGL((rd_lstm_mfma_f32_kernel<2, 0>), grid, blk, 0, st, m->d, rb, logits, labels); break;
#ifdef RD_DIAG
        case 10: hipLaunchKernelGGL((rd_lstm_mfma_f32_kernel<0, 0>), grid, blk, 0, st, m->d, rb, logits, labels); break;
        case 11: hipLaunchKernelGGL((rd_lstm_mfma_f32_kernel<1, 0>), grid, blk, 0, st, m->d, rb, logits, labels); break;
        case 12: hipLaunchKernelGGL((rd_lstm_mfma_f32_kernel<0, 1>), grid, blk, 0, st, m->d, rb, logits, labels); break;
        case 13: hipLaunchKernelGGL((rd_lstm_mfma_f32_kernel<1, 1>), grid, blk, 0, st, m->d, rb, logits, labels); break;
        case 20: hipLaunchKernelGGL((rd_lstm_mfma_f32_kernel<1, 0, 1>), grid, blk, 0, st, m->d, rb, logits, labels); break;
        case 21: hipLaunchKernelGGL((rd_lstm_mfma_f32_kernel<1, 0, 2>), grid, blk, 0, st, m->d, rb, logits, labels); break;
        case 22: hipLaunchKernelGGL((rd_lstm_mfma_f32_kernel<1, 0, 3>), grid, blk, 0, st, m->d, rb, logits, labels); break;
        case 23: hipLaunchKernelGGL((rd_lstm_mfma_f32_kernel<1, 0, 4>), grid, blk, 0, st, m->d, rb, logits, labels); break;
#endif
        default: RD_FAIL(RD_E_UNSUPPORTED, "rd_classify: variant %d not available in this build", m->variant);
        }
    }
    RD_HIP(hipGetLastError());
    if (ev) { RD_HIP(hipEventRecord(ev[1], st)); m->prof_count++; }
    if (join_after_launch >= 0) {   // everything issued on `st` from here on sees the final results of the group just evaluated
        rc = rd_async_join(m, st, join_after_launch);
        if (rc) return rc;
    }
    if (m->refine_thresh > 0.0f) {
        if (!deferred) return rd_refine_launch(m, rb, logits, labels, nullptr, m->refine_thresh, st);
        auto &pd = m->q_pend[m->q_cur][m->q_npend[m->q_cur]++];   // (the recurrence kernel's epilogue recorded the candidates)
        pd.p[0] = arena; pd.p[1] = seq_off; pd.p[2] = seq_len; pd.p[3] = logits; pd.p[4] = labels;
        pd.n = n; pd.max_len = max_len; pd.sem = m->semantics; pd.thresh = m->refine_thresh;
        m->q_calls++;
    }
    return RD_OK;
}

int rd_pair_fuse(const float *logits1, const float *logits2, int64_t n, int32_t ensure_mode, int8_t *pair_labels,
                 uint64_t *counts, void *stream) {
    if (n < 0 || ensure_mode < 0 || ensure_mode > 3) RD_FAIL(RD_E_INVALID, "rd_pair_fuse: bad n or ensure_mode");
    if (n == 0) return RD_OK;
    if (!logits1 || !logits2 || !pair_labels) RD_FAIL(RD_E_INVALID, "rd_pair_fuse: null pointer");
    // few, fat workgroups: every workgroup ends with three global atomics on the same counters
    int64_t nb = (n + 2047) / 2048;
    if (nb > 1024) nb = 1024;
    const bool vec = (((uintptr_t)logits1 | (uintptr_t)logits2) & 15) == 0 && ((uintptr_t)pair_labels & 1) == 0;
    if (vec)
        hipLaunchKernelGGL(rd_pair_fuse_kernel<true>, dim3((unsigned)nb), dim3(256), 0, (hipStream_t)stream, (const float2 *)logits1,
                           (const float2 *)logits2, n, ensure_mode, pair_labels, counts);
    else
        hipLaunchKernelGGL(rd_pair_fuse_kernel<false>, dim3((unsigned)nb), dim3(256), 0, (hipStream_t)stream, (const float2 *)logits1,
                           (const float2 *)logits2, n, ensure_mode, pair_labels, counts);
    RD_HIP(hipGetLastError());
    return RD_OK;
}

int rd_count_labels(const uint8_t *labels, int64_t n, uint64_t *counts, void *stream) {
    if (n < 0) RD_FAIL(RD_E_INVALID, "rd_count_labels: bad n");
    if (n == 0) return RD_OK;
    if (!labels || !counts) RD_FAIL(RD_E_INVALID, "rd_count_labels: null pointer");
    int64_t nb = (n + 16383) / 16384;
    if (nb > 1024) nb = 1024;
    if (((uintptr_t)labels & 15) == 0)
        hipLaunchKernelGGL(rd_count_kernel<true>, dim3((unsigned)nb), dim3(256), 0, (hipStream_t)stream, labels, n, counts);
    else
        hipLaunchKernelGGL(rd_count_kernel<false>, dim3((unsigned)nb), dim3(256), 0, (hipStream_t)stream, labels, n, counts);
    RD_HIP(hipGetLastError());
    return RD_OK;
}

int rd_encode_codes(const uint8_t *arena, const int64_t *seq_off, const int32_t *seq_len, int64_t n, int32_t max_len,
                    int32_t stride, uint8_t *codes, void *stream) {
    if (n < 0 || max_len < 1 || stride < max_len) RD_FAIL(RD_E_INVALID, "rd_encode_codes: bad n/max_len/stride");
    if (n == 0) return RD_OK;
    if (!arena || !seq_off || !seq_len || !codes) RD_FAIL(RD_E_INVALID, "rd_encode_codes: null pointer");
    if ((int64_t)ENC_R * stride > 0x7fffffffLL) RD_FAIL(RD_E_INVALID, "rd_encode_codes: stride too large");
    int64_t nb = (n + ENC_R - 1) / ENC_R;
    if (nb > 256 * 64) nb = 256 * 64;
    if (((uintptr_t)codes & 3) == 0 && (stride & 3) == 0)   // every piece of every row starts on a dword boundary
        hipLaunchKernelGGL(rd_encode_codes_kernel<true>, dim3((unsigned)nb), dim3(256), 0, (hipStream_t)stream, arena, seq_off, seq_len,
                           n, max_len, stride, codes);
    else
        hipLaunchKernelGGL(rd_encode_codes_kernel<false>, dim3((unsigned)nb), dim3(256), 0, (hipStream_t)stream, arena, seq_off, seq_len,
                           n, max_len, stride, codes);
    RD_HIP(hipGetLastError());
    return RD_OK;
}

int rd_encode_onehot_padded(const uint8_t *arena, const int64_t *seq_off, const int32_t *seq_len, int64_t n,
                            int32_t max_len, float *onehot, void *stream) {
    if (n < 0 || max_len < 1) RD_FAIL(RD_E_INVALID, "rd_encode_onehot_padded: bad n/max_len");
    if (n == 0) return RD_OK;
    if (!arena || !seq_off || !seq_len || !onehot) RD_FAIL(RD_E_INVALID, "rd_encode_onehot_padded: null pointer");
    if (max_len > MAX_LEN_LIMIT) RD_FAIL(RD_E_INVALID, "rd_encode_onehot_padded: max_len=%d out of range [1,%d]", max_len, MAX_LEN_LIMIT);
    int64_t nb = (n + ENC_R - 1) / ENC_R;
    if (nb > 256 * 64) nb = 256 * 64;
    hipLaunchKernelGGL(rd_encode_onehot_padded_kernel, dim3((unsigned)nb), dim3(256), 0, (hipStream_t)stream, arena, seq_off,
                       seq_len, n, max_len, (f32x4 *)onehot);
    RD_HIP(hipGetLastError());
    return RD_OK;
}

int rd_pack_plan(const int32_t *seq_len, int64_t n, int32_t max_len, int64_t *sorted_idx, int64_t *unsorted_idx,
                 int64_t *batch_sizes, int64_t *total_steps, void *workspace, size_t workspace_bytes, void *stream) {
    if (n < 1 || max_len < 1 || max_len > MAX_LEN_LIMIT) RD_FAIL(RD_E_INVALID, "rd_pack_plan: bad n/max_len");
    if (!seq_len || !sorted_idx || !unsorted_idx || !batch_sizes || !total_steps || !workspace)
        RD_FAIL(RD_E_INVALID, "rd_pack_plan: null pointer");
    int32_t *order = nullptr;
    int64_t *len_start = nullptr;
    return run_sort(seq_len, n, max_len, workspace, workspace_bytes, order, sorted_idx, unsorted_idx, batch_sizes, total_steps,
                    len_start, (hipStream_t)stream);
}

int rd_pack_onehot(const uint8_t *arena, const int64_t *seq_off, const int32_t *seq_len, int64_t n, int32_t max_len,
                   const int64_t *sorted_idx, const int64_t *batch_sizes, float *data, void *stream) {
    if (n < 1 || max_len < 1) RD_FAIL(RD_E_INVALID, "rd_pack_onehot: bad n/max_len");
    if (!arena || !seq_off || !seq_len || !sorted_idx || !batch_sizes || !data) RD_FAIL(RD_E_INVALID, "rd_pack_onehot: null pointer");
    hipStream_t st = (hipStream_t)stream;
    const int64_t nb = (n + ENC_R - 1) / ENC_R;
    if (nb > 0x7fffffffLL) RD_FAIL(RD_E_INVALID, "rd_pack_onehot: n too large");
    hipLaunchKernelGGL(rd_pack_onehot_kernel, dim3((unsigned)nb), dim3(256), 0, st, arena, seq_off, seq_len, n, max_len, sorted_idx,
                       batch_sizes, (f32x4 *)data);
    RD_HIP(hipGetLastError());
    return RD_OK;
}

// ---- device-side gzip of the label-partitioned records (rd_deflate.hpp) ------------------------------------------------------------
namespace {
// the member stage of both gzip entry points: the stream to deflate (member m starts at plain + 65,280 m), the token scratch of the
// deflate kernel's workgroups, a slot and a size per member, the members' offsets in `out`
struct GzMembers {
    int64_t cap_members;    // members the stream can have at most
    int grid;               // workgroups of the deflate kernel
    uint8_t *plain, *slots;
    uint32_t *toks, *msize;
    int64_t *moff;
};
GzMembers gz_members(Carver &c, int64_t cap_members) {
    GzMembers m{cap_members, (int)(cap_members < GZ_MAX_GRID ? cap_members : GZ_MAX_GRID)};
    m.plain = c.take<uint8_t>((size_t)cap_members * GZ_MEMBER + 256);
    m.toks = c.take<uint32_t>((size_t)m.grid * GZ_MEMBER);
    m.slots = c.take<uint8_t>((size_t)cap_members * GZ_SLOT);
    m.msize = c.take<uint32_t>((size_t)cap_members);
    m.moff = c.take<int64_t>((size_t)cap_members);
    return m;
}
// the members of m.plain (their lengths: ml) deflated, and compacted into `out`; info = (compressed bytes, text bytes, members, fault)
extern "C++" template <class MemberLen>      // (inside the C ABI's extern "C": a template needs C++ linkage)
void gz_deflate_members(const GzMembers &m, const MemberLen ml, int64_t *info, uint8_t *out, size_t out_cap, hipStream_t st) {
    hipLaunchKernelGGL(rd_gz_deflate_kernel<MemberLen>, dim3(m.grid), dim3(GZ_THREADS), 0, st, m.plain, ml, m.toks, m.slots, m.msize);
    hipLaunchKernelGGL(rd_gz_moff_kernel, dim3(1), dim3(256), 0, st, m.msize, m.moff, info);
    hipLaunchKernelGGL(rd_gz_compact_kernel, dim3(m.grid), dim3(256), 0, st, m.slots, m.msize, m.moff, info, out, (int64_t)out_cap);
}

// What the four pack entry points (`fn`) refuse, and their n == 0 answer (info zeroed; the grouped ones - key_tab's K rows belong to
// them - zero the keys' table too). `sel`: the labels or the keys; `need`: the bytes of the caller's workspace; `out` must be
// out_align-byte aligned. The caller goes on only when this returned RD_OK and n > 0.
int pack_check(const char *fn, bool grouped, const uint8_t *text, int64_t text_bytes, const int64_t *rec_start, const void *sel, int64_t n, int32_t label_or_K,
               const uint8_t *out, unsigned out_align, int64_t *key_tab, int64_t *info, const void *workspace, size_t workspace_bytes, size_t need, hipStream_t st) {
    if (n < 0 || n > 0x7fffffffLL || text_bytes < 0) RD_FAIL(RD_E_INVALID, "%s: bad n or text_bytes", fn);
    if (grouped && (label_or_K < 1 || label_or_K > RD_GROUP_KEYS_MAX)) RD_FAIL(RD_E_INVALID, "%s: K = %d is outside 1..%d", fn, label_or_K, RD_GROUP_KEYS_MAX);
    if (!info || (grouped && !key_tab)) RD_FAIL(RD_E_INVALID, grouped ? "%s: null info or key_tab" : "%s: null info", fn);
    if (!grouped && (label_or_K < -128 || label_or_K > 127)) RD_FAIL(RD_E_INVALID, "%s: label %d is not an int8 value", fn, label_or_K);
    if (n == 0) {
        RD_HIP(hipMemsetAsync(info, 0, 4 * sizeof(int64_t), st));
        if (grouped) RD_HIP(hipMemsetAsync(key_tab, 0, (size_t)label_or_K * 4 * sizeof(int64_t), st));
        return RD_OK;
    }
    if ((!text && text_bytes > 0) || !rec_start || !sel || !out || !workspace) RD_FAIL(RD_E_INVALID, "%s: null pointer", fn);
    if (((uintptr_t)workspace & 255) || ((uintptr_t)out & (out_align - 1)))
        RD_FAIL(RD_E_INVALID, "%s: workspace must be 256-byte aligned, out %u-byte aligned", fn, out_align);
    if (workspace_bytes < need) RD_FAIL(RD_E_WORKSPACE, "%s: workspace too small: %zu < %zu", fn, workspace_bytes, need);
    return RD_OK;
}

// the workspace of rd_gz_compress_selected; its head, the selection scan's part, is all of rd_select_pack's. Sizes that the entry
// points refuse (n < 0, text_bytes < 0) give an empty layout: total = 0, what the *_workspace_bytes functions answer to them
struct GzWs {
    int nb;                 // scan blocks
    int64_t *out_off, *bsum;
    GzMembers m;            // at most (text_bytes + 65,279) / 65,280 members: every record selected
    size_t sel_total, total;    // sel_total: the bytes of out_off + bsum, the selection scan's part
};
GzWs gz_ws(void *workspace, int64_t n, int64_t text_bytes) {
    GzWs p{};
    if (n < 0 || text_bytes < 0) return p;
    Carver c(workspace);
    p.nb = scan_blocks(n);
    p.out_off = c.take<int64_t>((size_t)(n + 1));
    p.bsum = c.take<int64_t>((size_t)p.nb);
    p.sel_total = c.off;
    const int64_t cap_members = (text_bytes + GZ_MEMBER - 1) / GZ_MEMBER;
    p.m = gz_members(c, cap_members < 1 ? 1 : cap_members);
    p.total = c.off;
    return p;
}

// What rd_gz_compress_selected and rd_select_pack (`fn`) share: pack_check, and the selection scan that packs the selected records
// into `dst` (more selected bytes than `limit`: info[3] = 1, nothing packed). The caller goes on only when n > 0.
int sel_scan_pack(const char *fn, const uint8_t *text, int64_t text_bytes, const int64_t *rec_start, const int8_t *labels, int64_t n, int32_t label,
                  const uint8_t *out, unsigned out_align, int64_t *info, const void *workspace, size_t workspace_bytes, size_t need, const GzWs &s,
                  uint8_t *dst, int64_t limit, hipStream_t st) {
    const int rc = pack_check(fn, false, text, text_bytes, rec_start, labels, n, label, out, out_align, nullptr, info, workspace, workspace_bytes, need, st);
    if (rc || n == 0) return rc;
    const GzSelLen len = {rec_start, labels, (int)label};
    hipLaunchKernelGGL((rd_scan_sum_kernel<8, GzSelLen>), dim3(s.nb), dim3(256), 0, st, len, n, s.bsum);
    // info[3] != 0: the record table does not describe the text (rd_gz_compress_selected's limit is the text's bytes: more selected
    // bytes than that are overlapping or stray records) - the workspace is sized by the text, so nothing is packed or compressed
    scan_base(s.bsum, s.nb, info, limit, st, GZ_MEMBER);
    hipLaunchKernelGGL((rd_scan_off_kernel<8, 1, GzSelLen, ScanNoVerdict>), dim3(s.nb), dim3(256), 0, st, len, n, ScanOut<1>{{s.out_off}, {s.bsum}}, ScanNoVerdict{});
    hipLaunchKernelGGL(rd_pack_kernel<GzSelPlaces>, dim3((unsigned)((n + GZ_PACK_RECS - 1) / GZ_PACK_RECS)), dim3(256), 0, st, text,
                       GzSelPlaces{rec_start, s.out_off, n}, dst, info);
    RD_HIP(hipGetLastError());
    return RD_OK;
}
}  // namespace

size_t rd_gz_workspace_bytes(int64_t n, int64_t text_bytes) {
    return gz_ws(nullptr, n, text_bytes).total;
}

size_t rd_gz_out_bound(int64_t text_bytes) {
    if (text_bytes < 0) return 0;
    const int64_t members = (text_bytes + GZ_MEMBER - 1) / GZ_MEMBER;
    return (size_t)members * (GZ_HDR + 5 + GZ_TRL) + (size_t)text_bytes;   // every member as a stored block
}

int rd_gz_eof_block(uint8_t *dst, size_t cap) {   // BGZF's end-of-file marker: an empty member (28 bytes)
    static const uint8_t eof[28] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    if (!dst || cap < sizeof(eof)) RD_FAIL(RD_E_INVALID, "rd_gz_eof_block: need 28 bytes");
    memcpy(dst, eof, sizeof(eof));
    return (int)sizeof(eof);
}

int rd_gz_compress_selected(const uint8_t *text, int64_t text_bytes, const int64_t *rec_start, const int8_t *labels, int64_t n,
                            int32_t label, uint8_t *out, size_t out_cap, int64_t *info, void *workspace, size_t workspace_bytes,
                            void *stream) {
    hipStream_t st = (hipStream_t)stream;
    const GzWs p = gz_ws(workspace, n, text_bytes);
    const int rc = sel_scan_pack("rd_gz_compress_selected", text, text_bytes, rec_start, labels, n, label, out, 256, info, workspace, workspace_bytes,
                                 p.total, p, p.m.plain, text_bytes, st);
    if (rc || n == 0) return rc;
    gz_deflate_members(p.m, GzStreamLen{info}, info, out, out_cap, st);
    RD_HIP(hipGetLastError());
    return RD_OK;
}

// the selected records of a chunk as one contiguous text (the selection scan and the pack kernel of the device gzip, without the deflate)
size_t rd_select_workspace_bytes(int64_t n) {
    return gz_ws(nullptr, n, 0).sel_total;
}

int rd_select_pack(const uint8_t *text, int64_t text_bytes, const int64_t *rec_start, const int8_t *labels, int64_t n, int32_t label, uint8_t *out,
                   size_t out_cap, int64_t *info, void *workspace, size_t workspace_bytes, void *stream) {
    const GzWs p = gz_ws(workspace, n, 0);
    const int64_t limit = text_bytes < (int64_t)out_cap ? text_bytes : (int64_t)out_cap;   // more selected bytes than text, or than `out` holds
    return sel_scan_pack("rd_select_pack", text, text_bytes, rec_start, labels, n, label, out, 16, info, workspace, workspace_bytes, p.sel_total, p, out, limit,
                         (hipStream_t)stream);
}

// ---- the records of a chunk partitioned by key: a run of text or of gzip members per key (rd_group_pack.hpp) -----------------------
namespace {
// the workspace of rd_group_pack (gz = false) and rd_gz_compress_grouped; bad arguments give an empty layout, total = 0
struct GpWs {
    GpParts parts;
    int64_t entries;        // K * parts: the (key, part) counters
    int nb_pos, nb_len;     // scan blocks over the counters, over the records
    int64_t *head;          // [0..3] the counters' scan, [4..7] the lengths' scan, [8] the fault flag of the count pass
    uint32_t *cnt, *gcur, *mlen;
    int64_t *pos, *bsum_pos, *L, *bsum_len, *shift;
    int32_t *perm;
    GzMembers m;            // gz: the padded stream's members, and mlen: their lengths
    size_t total;
};
GpWs gp_ws(void *workspace, int64_t n, int64_t text_bytes, int64_t K, bool gz) {
    GpWs p{};
    if (n < 0 || n > 0x7fffffffLL || text_bytes < 0 || K < 1 || K > RD_GROUP_KEYS_MAX) return p;
    Carver c(workspace);
    int64_t nb = (n + GP_PART_MIN - 1) / GP_PART_MIN;
    nb = nb < 1 ? 1 : nb > GP_MAX_PARTS ? GP_MAX_PARTS : nb;
    p.parts = GpParts{(int)nb, (n + nb - 1) / nb};
    p.entries = K * nb;
    p.nb_pos = scan_blocks(p.entries);
    p.nb_len = scan_blocks(n);
    p.head = c.take<int64_t>(16);
    p.cnt = c.take<uint32_t>((size_t)p.entries);
    p.gcur = c.take<uint32_t>(K > GP_LDS_KEYS ? (size_t)p.entries : 0);
    p.pos = c.take<int64_t>((size_t)p.entries + 1);
    p.bsum_pos = c.take<int64_t>((size_t)p.nb_pos);
    p.perm = c.take<int32_t>((size_t)n);
    p.L = c.take<int64_t>((size_t)n + 1);
    p.bsum_len = c.take<int64_t>((size_t)p.nb_len);
    p.shift = c.take<int64_t>((size_t)K);
    if (gz) {   // the padded stream: every key's run starts a member, so it holds text_bytes + 65,280 * min(K, n) bytes at most
        p.m = gz_members(c, text_bytes / GZ_MEMBER + (K < n ? K : n) + 1);
        p.mlen = c.take<uint32_t>((size_t)p.m.cap_members);
    }
    p.total = c.off;
    return p;
}

// What rd_group_pack and rd_gz_compress_grouped (`fn`) share: pack_check, the partition, the length scan, the keys' table and the
// pack into `dst`. The caller goes on only when n > 0.
int group_scan_pack(bool gz, const char *fn, const uint8_t *text, int64_t text_bytes, const int64_t *rec_start, const int32_t *keys, int64_t n, int32_t K,
                    const uint8_t *out, size_t out_cap, unsigned out_align, int64_t *key_tab, int64_t *info, void *workspace, size_t workspace_bytes,
                    const GpWs &p, uint8_t *dst, hipStream_t st) {
    const int rc = pack_check(fn, true, text, text_bytes, rec_start, keys, n, K, out, out_align, key_tab, info, workspace, workspace_bytes, p.total, st);
    if (rc || n == 0) return rc;
    const bool lds = K <= GP_LDS_KEYS;
    uint32_t *flag = reinterpret_cast<uint32_t *>(p.head + 8);
    int64_t *pinfo = p.head, *linfo = p.head + 4;
    RD_HIP(hipMemsetAsync(p.head, 0, 16 * sizeof(int64_t), st));
    if (!lds) RD_HIP(hipMemsetAsync(p.gcur, 0, (size_t)p.entries * sizeof(uint32_t), st));
    if (lds)
        hipLaunchKernelGGL(rd_gp_count_kernel<true>, dim3(p.parts.nb), dim3(64), 0, st, keys, rec_start, n, text_bytes, (int)K, p.parts, p.cnt, p.gcur, flag);
    else
        hipLaunchKernelGGL(rd_gp_count_kernel<false>, dim3(p.parts.nb), dim3(64), 0, st, keys, rec_start, n, text_bytes, (int)K, p.parts, p.cnt, p.gcur, flag);
    const GpCntLen clen = {p.cnt};
    hipLaunchKernelGGL((rd_scan_sum_kernel<8, GpCntLen>), dim3(p.nb_pos), dim3(256), 0, st, clen, p.entries, p.bsum_pos);
    scan_base(p.bsum_pos, p.nb_pos, pinfo, n, st);
    hipLaunchKernelGGL((rd_scan_off_kernel<8, 1, GpCntLen, ScanNoVerdict>), dim3(p.nb_pos), dim3(256), 0, st, clen, p.entries, ScanOut<1>{{p.pos}, {p.bsum_pos}}, ScanNoVerdict{});
    if (lds)
        hipLaunchKernelGGL(rd_gp_scatter_kernel<true>, dim3(p.parts.nb), dim3(64), 0, st, keys, n, (int)K, p.parts, p.pos, p.gcur, flag, p.perm);
    else
        hipLaunchKernelGGL(rd_gp_scatter_kernel<false>, dim3(p.parts.nb), dim3(64), 0, st, keys, n, (int)K, p.parts, p.pos, p.gcur, flag, p.perm);
    // more bytes in the keyed records than in the text: overlapping records - the table does not describe the text (linfo[3])
    const GpPermLen plen = {p.perm, rec_start, p.pos + p.entries, flag};
    hipLaunchKernelGGL((rd_scan_sum_kernel<8, GpPermLen>), dim3(p.nb_len), dim3(256), 0, st, plen, n, p.bsum_len);
    scan_base(p.bsum_len, p.nb_len, linfo, text_bytes, st);
    hipLaunchKernelGGL((rd_scan_off_kernel<8, 1, GpPermLen, ScanNoVerdict>), dim3(p.nb_len), dim3(256), 0, st, plen, n, ScanOut<1>{{p.L}, {p.bsum_len}}, ScanNoVerdict{});
    if (gz) {
        hipLaunchKernelGGL(rd_gp_keytab_kernel<true>, dim3(1), dim3(256), 0, st, p.pos, p.L, (int)K, p.parts.nb, flag, linfo, (int64_t)out_cap, p.shift, key_tab, info);
        hipLaunchKernelGGL(rd_gp_mlen_kernel, dim3((unsigned)(K < 1024 ? K : 1024)), dim3(256), 0, st, key_tab, (int)K, p.mlen, info);
    } else {
        hipLaunchKernelGGL(rd_gp_keytab_kernel<false>, dim3(1), dim3(256), 0, st, p.pos, p.L, (int)K, p.parts.nb, flag, linfo, (int64_t)out_cap, p.shift, key_tab, info);
    }
    hipLaunchKernelGGL(rd_pack_kernel<GpPermPlaces>, dim3((unsigned)((n + GZ_PACK_RECS - 1) / GZ_PACK_RECS)), dim3(256), 0, st, text,
                       GpPermPlaces{rec_start, keys, p.perm, p.L, p.shift, p.pos + p.entries}, dst, info);
    RD_HIP(hipGetLastError());
    return RD_OK;
}
}  // namespace

int rd_group_keys(const int32_t *rows, int64_t first, int64_t stride, int32_t mate, const int8_t *labels, int64_t n, const int32_t *class_slot, int32_t G,
                  int32_t *keys, int64_t *info, void *stream) {
    if (n < 0 || n > 0x3fffffffLL || G < 0 || G > RD_SPLIT_GROUPS_MAX) RD_FAIL(RD_E_INVALID, "rd_group_keys: bad n or G");
    if (first < 0 || stride < 1) RD_FAIL(RD_E_INVALID, "rd_group_keys: bad first / stride");
    if (mate < -1 || mate > 1) RD_FAIL(RD_E_INVALID, "rd_group_keys: mate must be -1 (a key per unit), 0 or 1; got %d", mate);
    if (!class_slot || !info) RD_FAIL(RD_E_INVALID, "rd_group_keys: null class_slot or info");
    GpSlots slots;
    for (int c = 0; c < 3; ++c) {
        if (class_slot[c] < -1 || class_slot[c] > 2) RD_FAIL(RD_E_INVALID, "rd_group_keys: class_slot[%d] = %d is outside -1..2", c, class_slot[c]);
        slots.s[c] = class_slot[c];
    }
    RD_HIP(hipMemsetAsync(info, 0, 4 * sizeof(int64_t), (hipStream_t)stream));
    if (n == 0) return RD_OK;
    if (!rows || !labels || !keys) RD_FAIL(RD_E_INVALID, "rd_group_keys: null pointer");
    hipLaunchKernelGGL(rd_group_keys_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, rows, first, stride, (int)mate, labels, n, slots,
                       (int)G, keys, info);
    RD_HIP(hipGetLastError());
    return RD_OK;
}

size_t rd_group_workspace_bytes(int64_t n, int64_t text_bytes, int32_t K, int32_t gz) {
    return gp_ws(nullptr, n, text_bytes, K, gz != 0).total;
}

size_t rd_gz_grouped_out_bound(int64_t text_bytes, int32_t K) {
    if (text_bytes < 0 || K < 1 || K > RD_GROUP_KEYS_MAX) return 0;
    const int64_t members = text_bytes / GZ_MEMBER + K;     // every key may end in a short member
    return (size_t)members * (GZ_HDR + 5 + GZ_TRL) + (size_t)text_bytes;   // every member as a stored block
}

int rd_group_pack(const uint8_t *text, int64_t text_bytes, const int64_t *rec_start, const int32_t *keys, int64_t n, int32_t K, uint8_t *out, size_t out_cap,
                  int64_t *key_tab, int64_t *info, void *workspace, size_t workspace_bytes, void *stream) {
    const GpWs p = gp_ws(workspace, n, text_bytes, K, false);
    return group_scan_pack(false, "rd_group_pack", text, text_bytes, rec_start, keys, n, K, out, out_cap, 16, key_tab, info, workspace, workspace_bytes, p, out,
                                  (hipStream_t)stream);
}

int rd_gz_compress_grouped(const uint8_t *text, int64_t text_bytes, const int64_t *rec_start, const int32_t *keys, int64_t n, int32_t K, uint8_t *out,
                           size_t out_cap, int64_t *key_tab, int64_t *info, void *workspace, size_t workspace_bytes, void *stream) {
    hipStream_t st = (hipStream_t)stream;
    const GpWs p = gp_ws(workspace, n, text_bytes, K, true);
    const int rc = group_scan_pack(true, "rd_gz_compress_grouped", text, text_bytes, rec_start, keys, n, K, out, out_cap, 256, key_tab, info, workspace,
                                         workspace_bytes, p, p.m.plain, st);
    if (rc || n == 0) return rc;
    gz_deflate_members(p.m, GzTableLen{info, p.mlen}, info, out, out_cap, st);
    hipLaunchKernelGGL(rd_gp_keytab_gz_kernel, dim3((unsigned)((K + 255) / 256)), dim3(256), 0, st, p.m.moff, (int)K, (int64_t)out_cap, key_tab, info);
    RD_HIP(hipGetLastError());
    return RD_OK;
}

int rd_gz_inflate_members(const uint8_t *comp, int64_t comp_bytes, const rd_gz_member *members, int64_t n, uint8_t *text, int64_t text_bytes,
                          uint32_t *status, void *stream) {
    static_assert(sizeof(rd_gz_member) == sizeof(GzMemberIn), "rd_gz_member layout");
    if (n < 0 || comp_bytes < 0 || text_bytes < 0) RD_FAIL(RD_E_INVALID, "rd_gz_inflate_members: bad size");
    if (n == 0) return RD_OK;
    if (!comp || !members || !status || (!text && text_bytes > 0)) RD_FAIL(RD_E_INVALID, "rd_gz_inflate_members: null pointer");
    int64_t grid = (n + GZI_WAVES - 1) / GZI_WAVES;
    if (grid > 65536) grid = 65536;
    hipLaunchKernelGGL(rd_gz_inflate_kernel, dim3((unsigned)grid), dim3(64 * GZI_WAVES), 0, (hipStream_t)stream, comp, comp_bytes,
                       (const GzMemberIn *)members, n, text, text_bytes, status);
    RD_HIP(hipGetLastError());
    return RD_OK;
}

// ---- one DEFLATE stream inflated on the device (rd_inflate_stream.hpp): rd_gz_stream_inflate gives a batch's text as bytes behind the
// carried window; rd_gz_range_decode (a range of a stream) gives it as symbols, bytes once the window in front of the range is known
namespace {
size_t gzs_workspace_bytes(int64_t data_bytes, int32_t section_bytes, int32_t cap_syms, int64_t text_cap) {
    if (data_bytes < 0 || section_bytes < 1024 || cap_syms < 1024 || text_cap < 0) return 0;
    return gzs_ws(nullptr, data_bytes, section_bytes, cap_syms, text_cap).total;
}

// CRC-32 and length of text[0, S->n_text) folded into the state
void gzs_crc_fold(const uint8_t *text, int ctiles, GzsState *S, uint32_t *tcrc, hipStream_t st) {
    hipLaunchKernelGGL(rd_gzs_crc_kernel, dim3((unsigned)((ctiles + 3) / 4)), dim3(256), 0, st, text, S, tcrc);
    hipLaunchKernelGGL(rd_gzs_fold_kernel, dim3(1), dim3(64), 0, st, tcrc, S);
}

// One batch for both entry points (`fn`): validation, carve, block-start search, section decode, scan, then the window chain on symbols
// (the groups of sections side by side, then the groups in order) and the resolve pass. range = false: `carried_in` / `carried_out` are
// the 32 KiB window as bytes and `text_out` receives bytes, with their CRC; true: 16-bit maps and symbols, and no CRC yet.
int gzs_batch(const char *fn, bool range, const uint8_t *comp, int64_t comp_bytes, int64_t data_bytes, int64_t valid_bytes, int32_t section_bytes,
              int32_t cap_syms, uint32_t first_start_bit, const rd_gzs_state *carry, int64_t carry_delta_bits, int32_t at_eof, const void *carried_in,
              void *carried_out, void *text_out, int64_t text_cap, rd_gzs_state *state, void *workspace, size_t workspace_bytes, void *stream) {
    const char *out_name = range ? "sym_text" : "text";
    const unsigned out_align = range ? 16 : 8;
    if (!comp || !carried_out || !text_out || !state || !workspace) RD_FAIL(RD_E_INVALID, "%s: null pointer", fn);
    if (((uintptr_t)comp & 3) || ((uintptr_t)workspace & 255) || ((uintptr_t)text_out & (out_align - 1)))
        RD_FAIL(RD_E_INVALID, "%s: comp must be 4-byte aligned, %s %u-byte aligned, workspace 256-byte aligned", fn, out_name, out_align);
    if (data_bytes <= 0 || valid_bytes < data_bytes || comp_bytes < valid_bytes || valid_bytes >= (1LL << 28) || section_bytes < 1024 || (section_bytes & 3) ||
        cap_syms < 1024 || text_cap < 0)
        RD_FAIL(RD_E_INVALID, "%s: bad sizes (a batch holds < 256 MiB of compressed bytes)", fn);
    if (range && (carry == nullptr) != (carried_in == nullptr))
        RD_FAIL(RD_E_INVALID, "%s: carry and map_in go together (both null: the range's first batch)", fn);
    const GzsWs p = gzs_ws(workspace, data_bytes, section_bytes, cap_syms, text_cap);
    if (workspace_bytes < p.total) RD_FAIL(RD_E_WORKSPACE, "%s: workspace too small: %zu < %zu", fn, workspace_bytes, p.total);
    hipStream_t st = (hipStream_t)stream;
    const uint32_t end_bits = (uint32_t)(valid_bytes * 8), sec_bits = (uint32_t)section_bytes * 8u;
    GzsState *S = (GzsState *)state;
    const GzsState *C = (const GzsState *)carry;
    const int search0 = (range && C == nullptr && first_start_bit == GZS_SEARCH) ? 1 : 0;
    const dim3 resolve_grid((unsigned)(p.nsec * p.tiles_per_sec));
    hipLaunchKernelGGL(rd_gzs_search_kernel, dim3((unsigned)((p.nsec + 1 + GZS_WAVES - 1) / GZS_WAVES)), dim3(64 * GZS_WAVES), 0, st, comp, comp_bytes, end_bits, sec_bits,
                       p.nsec, first_start_bit, C, carry_delta_bits, p.found);
    hipLaunchKernelGGL(rd_gzs_decode_kernel, dim3((unsigned)((p.nsec + GZS_WAVES - 1) / GZS_WAVES)), dim3(64 * GZS_WAVES), 0, st, comp, comp_bytes, end_bits, p.nsec, p.found,
                       p.syms, (int)cap_syms, p.sec);
    hipLaunchKernelGGL(rd_gzs_scan_kernel, dim3(1), dim3(64), 0, st, p.sec, p.found, p.nsec, (int)at_eof, text_cap, p.off, p.wslot, p.plist, S, C, search0);
    hipLaunchKernelGGL(rd_gzs_symwin_kernel, dim3((unsigned)p.ngroups), dim3(1024), 0, st, p.syms, (int)cap_syms, p.sec, p.plist, p.wslot, p.nsec, S, p.windows16, p.gmaps);
    if (!range) {
        hipLaunchKernelGGL(rd_gzs_chain_kernel, dim3(1), dim3(1024), 0, st, p.gmaps, p.wslot, p.nsec, S, (const uint8_t *)carried_in, (const uint16_t *)nullptr, 1, p.gwin,
                           (uint16_t *)nullptr, (uint8_t *)carried_out);
        hipLaunchKernelGGL(rd_gzs_resolve_kernel<false>, resolve_grid, dim3(256), 0, st, p.syms, (int)cap_syms, p.sec, p.found, p.off, p.wslot, p.tiles_per_sec, p.windows16,
                           p.gwin, S, (uint8_t *)text_out, (uint16_t *)nullptr);
        gzs_crc_fold((const uint8_t *)text_out, p.ctiles, S, p.tcrc, st);
    } else {
        hipLaunchKernelGGL(rd_gzs_chain_kernel, dim3(1), dim3(1024), 0, st, p.gmaps, p.wslot, p.nsec, S, (const uint8_t *)nullptr, (const uint16_t *)carried_in, 0, p.gwin,
                           (uint16_t *)carried_out, (uint8_t *)nullptr);
        hipLaunchKernelGGL(rd_gzs_resolve_kernel<true>, resolve_grid, dim3(256), 0, st, p.syms, (int)cap_syms, p.sec, p.found, p.off, p.wslot, p.tiles_per_sec, p.windows16,
                           p.gwin, S, (uint8_t *)nullptr, (uint16_t *)text_out);
    }
    RD_HIP(hipGetLastError());
    return RD_OK;
}
}  // namespace

size_t rd_gz_stream_workspace_bytes(int64_t data_bytes, int32_t section_bytes, int32_t cap_syms, int64_t text_cap) {
    return gzs_workspace_bytes(data_bytes, section_bytes, cap_syms, text_cap);
}

int rd_gz_stream_inflate(const uint8_t *comp, int64_t comp_bytes, int64_t data_bytes, int64_t valid_bytes, int32_t section_bytes, int32_t cap_syms,
                         uint32_t first_start_bit, const rd_gzs_state *carry, int64_t carry_delta_bits, int32_t at_eof, const uint8_t *win_in,
                         uint8_t *win_out, uint8_t *text, int64_t text_cap, rd_gzs_state *state, void *workspace, size_t workspace_bytes, void *stream) {
    return gzs_batch("rd_gz_stream_inflate", false, comp, comp_bytes, data_bytes, valid_bytes, section_bytes, cap_syms, first_start_bit, carry, carry_delta_bits,
                     at_eof, win_in, win_out, text, text_cap, state, workspace, workspace_bytes, stream);
}

size_t rd_gz_range_workspace_bytes(int64_t data_bytes, int32_t section_bytes, int32_t cap_syms, int64_t text_cap) {
    return gzs_workspace_bytes(data_bytes, section_bytes, cap_syms, text_cap);
}

int rd_gz_range_decode(const uint8_t *comp, int64_t comp_bytes, int64_t data_bytes, int64_t valid_bytes, int32_t section_bytes, int32_t cap_syms,
                       uint32_t first_start_bit, const rd_gzs_state *carry, int64_t carry_delta_bits, int32_t at_eof, const uint16_t *map_in, uint16_t *map_out,
                       uint16_t *sym_text, int64_t text_cap, rd_gzs_state *state, void *workspace, size_t workspace_bytes, void *stream) {
    return gzs_batch("rd_gz_range_decode", true, comp, comp_bytes, data_bytes, valid_bytes, section_bytes, cap_syms, first_start_bit, carry, carry_delta_bits,
                     at_eof, map_in, map_out, sym_text, text_cap, state, workspace, workspace_bytes, stream);
}

size_t rd_gz_range_resolve_workspace_bytes(int64_t n) { return n < 0 ? 0 : ((size_t)(n / GZS_CTILE + 2) * 4 + 255) / 256 * 256; }

int rd_gz_range_resolve(const uint16_t *sym_text, int64_t n, const uint8_t *window, uint32_t win_valid, uint8_t *text, rd_gzs_state *state, void *workspace,
                        size_t workspace_bytes, void *stream) {
    if (n < 0 || !state || (n > 0 && (!sym_text || !text || !workspace))) RD_FAIL(RD_E_INVALID, "rd_gz_range_resolve: bad argument");
    if (win_valid > 0 && !window) RD_FAIL(RD_E_INVALID, "rd_gz_range_resolve: win_valid > 0 needs a window");
    if (((uintptr_t)sym_text & 15) || ((uintptr_t)text & 15)) RD_FAIL(RD_E_INVALID, "rd_gz_range_resolve: sym_text and text must be 16-byte aligned");
    if (workspace_bytes < rd_gz_range_resolve_workspace_bytes(n)) RD_FAIL(RD_E_WORKSPACE, "rd_gz_range_resolve: workspace too small");
    hipStream_t st = (hipStream_t)stream;
    GzsState *S = (GzsState *)state;
    int64_t grid = n / (8 * 256 * 4) + 1;
    if (grid > 4096) grid = 4096;
    hipLaunchKernelGGL(rd_gzs_symtext_kernel, dim3((unsigned)grid), dim3(256), 0, st, sym_text, n, window, win_valid, text, S);
    gzs_crc_fold(text, (int)((n + GZS_CTILE - 1) / GZS_CTILE) + 1, S, (uint32_t *)workspace, st);
    RD_HIP(hipGetLastError());
    return RD_OK;
}

// ---- streams restricted to a set of compute units --------------------------------------------------------------------------------------------
int rd_stream_create(int device, const uint32_t *cu_mask, int words, int priority, void **stream) {
    if (!stream || words < 0 || (words > 0 && !cu_mask)) RD_FAIL(RD_E_INVALID, "rd_stream_create: bad argument");
    RD_HIP(hipSetDevice(device));
    hipStream_t st = nullptr;
    if (words > 0) {
        RD_HIP(hipExtStreamCreateWithCUMask(&st, (uint32_t)words, cu_mask));      // (no priority argument in this entry point: default priority)
    } else {
        int lo = 0, hi = 0;
        RD_HIP(hipDeviceGetStreamPriorityRange(&lo, &hi));
        RD_HIP(hipStreamCreateWithPriority(&st, hipStreamNonBlocking, priority < 0 ? hi : lo));
    }
    *stream = (void *)st;
    return RD_OK;
}

int rd_stream_destroy(void *stream) {
    if (stream) RD_HIP(hipStreamDestroy((hipStream_t)stream));
    return RD_OK;
}

int rd_copy_bytes(void *dst, const void *src, int64_t n, int32_t workgroups, void *stream) {
    if (n < 0 || (n > 0 && (!dst || !src))) RD_FAIL(RD_E_INVALID, "rd_copy_bytes: bad argument");
    if (n == 0) return RD_OK;
    int64_t grid = workgroups > 0 ? workgroups : 8;
    const int64_t need = n / (16 * COPY_THREADS) + 1;
    if (grid > need) grid = need;
    hipLaunchKernelGGL(rd_copy_kernel, dim3((unsigned)grid), dim3(COPY_THREADS), 0, (hipStream_t)stream, (uint8_t *)dst, (const uint8_t *)src, n);
    RD_HIP(hipGetLastError());
    return RD_OK;
}

// ---- FASTQ record index on the device, FASTA batches re-written and indexed (rd_fastq_index.hpp, which ends in the host code the two share; rd_fasta_index.hpp)
size_t rd_fastq_index_workspace_bytes(int64_t text_end) {
    if (text_end < 0 || text_end >= 0x7fffffffLL) return 0;
    return fq_ws(nullptr, text_end).total;
}

int rd_fastq_index(uint8_t *text, int64_t pad, int64_t end, const uint8_t *prev_text, const rd_fq_summary *prev, int32_t final, int32_t *line_end,
                   int64_t cap_lines, rd_fq_summary *summary, void *workspace, size_t workspace_bytes, void *stream) {
    if (const int rc = fq_index_check("rd_fastq_index", text, pad, end, prev_text, prev, line_end, cap_lines, summary, workspace, false, false, nullptr)) return rc;
    const FqWs p = fq_ws(workspace, end);
    if (workspace_bytes < p.total) RD_FAIL(RD_E_WORKSPACE, "rd_fastq_index: workspace too small: %zu < %zu", workspace_bytes, p.total);
    hipStream_t st = (hipStream_t)stream;
    FqSummary *sum = (FqSummary *)summary;
    fq_line_table(text, pad, end, prev_text, prev, final, line_end, cap_lines, sum, p, st);
    int grid = (int)((end - pad) / (64 * FQ_THREADS)) + 1;      // one thread per ~64 bytes of new text is more than one per record
    if (grid > 2048) grid = 2048;
    hipLaunchKernelGGL(rd_fq_check_kernel, dim3(grid), dim3(FQ_THREADS), 0, st, text, line_end, sum, (int)final);
    hipLaunchKernelGGL(rd_fq_verdict_kernel, dim3(1), dim3(1), 0, st, sum);
    RD_HIP(hipGetLastError());
    return RD_OK;
}

int rd_fastq_gather(const uint8_t *text, const int32_t *line_end, const rd_fq_summary *summary, int64_t rec_lo, int64_t rec_hi, int64_t max_bytes,
                    uint8_t *out_text, int64_t out_cap, const int64_t *cursor_in, int64_t *cursor_out, int64_t *rec_start, int64_t *seq_off,
                    int32_t *seq_len, void *stream) {
    return fq_gather("rd_fastq_gather", rd_fq_gather_kernel, summary, rec_lo, rec_hi, max_bytes, out_text, out_cap, cursor_in, cursor_out, rec_start, seq_off, seq_len,
                     stream, text, line_end);
}

int rd_fastq_sample(const int32_t *line_end, const rd_fq_summary *summary, int64_t every, int32_t *samples, int64_t cap, void *stream) {
    return fq_sample("rd_fastq_sample", rd_fq_sample_kernel, line_end, summary, every, samples, cap, stream);
}

int rd_fastq_strip_mark(const uint8_t *text, const int32_t *line_end, const rd_fq_summary *summary, int64_t max_lines, uint8_t *del, void *stream) {
    if (!text || !line_end || !summary || !del || max_lines < 0) RD_FAIL(RD_E_INVALID, "rd_fastq_strip_mark: bad argument");
    int64_t grid = max_lines / FQ_THREADS + 1;
    if (grid > 4096) grid = 4096;
    hipLaunchKernelGGL(rd_fq_strip_mark_kernel, dim3((unsigned)grid), dim3(FQ_THREADS), 0, (hipStream_t)stream, text, line_end, (const FqSummary *)summary, del);
    RD_HIP(hipGetLastError());
    return RD_OK;
}

size_t rd_fasta_index_workspace_bytes(int64_t text_end, int64_t cap_lines) {
    if (text_end < 0 || text_end >= 0x7fffffffLL || cap_lines < 0) return 0;
    return fa_ws(nullptr, text_end, cap_lines).total;
}

int rd_fasta_index(uint8_t *text, int64_t pad, int64_t end, const uint8_t *prev_text, const rd_fq_summary *prev, int32_t final, int32_t *line_end,
                   int64_t cap_lines, uint8_t *norm, int64_t norm_cap, int64_t *rec_tab, int32_t *hdr_tab, int64_t cap_records, rd_fq_summary *summary,
                   void *workspace, size_t workspace_bytes, void *stream) {
    if (const int rc = fq_index_check("rd_fasta_index", text, pad, end, prev_text, prev, line_end, cap_lines, summary, workspace, !norm || !rec_tab || !hdr_tab,
                                      norm_cap < 0 || cap_records < 1, norm))
        return rc;
    const FaWs p = fa_ws(workspace, end, cap_lines);
    if (workspace_bytes < p.total) RD_FAIL(RD_E_WORKSPACE, "rd_fasta_index: workspace too small: %zu < %zu", workspace_bytes, p.total);
    hipStream_t st = (hipStream_t)stream;
    FqSummary *sum = (FqSummary *)summary;
    fq_line_table(text, pad, end, prev_text, prev, final, line_end, cap_lines, sum, p.fq, st);
    hipLaunchKernelGGL(rd_fa_init_kernel, dim3(1), dim3(FQ_THREADS), 0, st, p.sc);
    hipLaunchKernelGGL(rd_fa_lines_kernel, dim3(p.nblk), dim3(FQ_THREADS), 0, st, text, line_end, sum, p.info_a, p.info_k, p.blk, p.sc);
    hipLaunchKernelGGL(rd_fa_base_kernel, dim3(1), dim3(FQ_THREADS), 0, st, p.blk, line_end, sum, p.sc, (int)final, norm_cap, cap_records, norm, rec_tab, hdr_tab);
    hipLaunchKernelGGL(rd_fa_emit_kernel, dim3(p.nblk), dim3(FQ_THREADS), 0, st, text, p.info_a, p.info_k, p.blk, sum, p.sc, (int)final, norm, rec_tab, hdr_tab);
    RD_HIP(hipGetLastError());
    return RD_OK;
}

int rd_fasta_gather(const uint8_t *norm, const int64_t *rec_tab, const int32_t *hdr_tab, const rd_fq_summary *summary, int64_t rec_lo, int64_t rec_hi,
                    int64_t max_bytes, uint8_t *out_text, int64_t out_cap, const int64_t *cursor_in, int64_t *cursor_out, int64_t *rec_start,
                    int64_t *seq_off, int32_t *seq_len, void *stream) {
    return fq_gather("rd_fasta_gather", rd_fa_gather_kernel<false>, summary, rec_lo, rec_hi, max_bytes, out_text, out_cap, cursor_in, cursor_out, rec_start, seq_off, seq_len,
                     stream, norm, rec_tab, hdr_tab);
}

int rd_fasta_sample(const int64_t *rec_tab, const rd_fq_summary *summary, int64_t every, int32_t *samples, int64_t cap, void *stream) {
    return fq_sample("rd_fasta_sample", rd_fa_sample_kernel<false>, rec_tab, summary, every, samples, cap, stream);
}

// ---- BAM records framed and re-written as FASTQ text (rd_bam_index.hpp)
size_t rd_bam_index_workspace_bytes(int64_t text_end) {
    if (text_end < 0 || text_end >= 0x7fffffffLL) return 0;
    return bam_ws(nullptr, text_end).total;
}

int rd_bam_index(uint8_t *text, int64_t pad, int64_t end, const uint8_t *prev_text, const rd_fq_summary *prev, int32_t final, uint8_t *norm, int64_t norm_cap,
                 int64_t *rec_tab, int32_t *hdr_tab, int64_t cap_records, rd_fq_summary *summary, void *workspace, size_t workspace_bytes, void *stream) {
    // (no line table: `text` stands in for it in the checks the three formats share)
    if (const int rc = fq_index_check("rd_bam_index", text, pad, end, prev_text, prev, (const int32_t *)text, 0, summary, workspace, !norm || !rec_tab || !hdr_tab,
                                      norm_cap < 0 || cap_records < 1, norm))
        return rc;
    const BamWs p = bam_ws(workspace, end);
    if (workspace_bytes < p.total) RD_FAIL(RD_E_WORKSPACE, "rd_bam_index: workspace too small: %zu < %zu", workspace_bytes, p.total);
    hipStream_t st = (hipStream_t)stream;
    FqSummary *sum = (FqSummary *)summary;
    hipLaunchKernelGGL(rd_fq_begin_kernel<false>, dim3(1), dim3(FQ_THREADS), 0, st, text, pad, end, prev_text, (const FqSummary *)prev, (int)final, sum);
    hipLaunchKernelGGL(rd_bam_walk_kernel<true>, dim3(p.nseg), dim3(64), 0, st, text, sum, p.seg, p.lists);
    hipLaunchKernelGGL(rd_bam_stitch_kernel<true>, dim3(1), dim3(64), 0, st, text, sum, p.seg, p.lists, p.nseg, p.seg_rbase, p.seg_nbase, p.seg_cnt, p.sc, (int)final, norm_cap,
                       cap_records, rec_tab);
    hipLaunchKernelGGL(rd_bam_table_kernel, dim3(p.nseg), dim3(64), 0, st, text, sum, p.sc, p.lists, p.seg_rbase, p.seg_nbase, p.seg_cnt, rec_tab, hdr_tab, p.src_tab);
    int64_t grid = (4 * end / 3 + 64) / BAM_EMIT_BYTES + 1;      // (the text of a window is at most 4 / 3 of its bytes)
    if (grid > 65536) grid = 65536;
    hipLaunchKernelGGL(rd_bam_emit_kernel, dim3((unsigned)grid), dim3(FQ_THREADS), 0, st, text, sum, rec_tab, p.src_tab, norm, norm_cap);
    RD_HIP(hipGetLastError());
    return RD_OK;
}

int rd_bam_gather(const uint8_t *norm, const int64_t *rec_tab, const int32_t *hdr_tab, const rd_fq_summary *summary, int64_t rec_lo, int64_t rec_hi,
                  int64_t max_bytes, uint8_t *out_text, int64_t out_cap, const int64_t *cursor_in, int64_t *cursor_out, int64_t *rec_start,
                  int64_t *seq_off, int32_t *seq_len, void *stream) {
    return fq_gather("rd_bam_gather", rd_fa_gather_kernel<true>, summary, rec_lo, rec_hi, max_bytes, out_text, out_cap, cursor_in, cursor_out, rec_start, seq_off, seq_len,
                     stream, norm, rec_tab, hdr_tab);
}

int rd_bam_sample(const int64_t *rec_tab, const rd_fq_summary *summary, int64_t every, int32_t *samples, int64_t cap, void *stream) {
    return fq_sample("rd_bam_sample", rd_fa_sample_kernel<true>, rec_tab, summary, every, samples, cap, stream);
}

// ---- a BAM file shared by the ranks of a run (rd_bam_shard.hpp)
int rd_bam_find_start(const uint8_t *text, int64_t lo, int64_t hi, int64_t end, int32_t at_eof, int64_t *info, void *stream) {
    if (!info || (!text && end > 0)) RD_FAIL(RD_E_INVALID, "rd_bam_find_start: null pointer");
    if ((uintptr_t)text & 15) RD_FAIL(RD_E_INVALID, "rd_bam_find_start: text must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const bool bad = lo < 0 || hi < lo || end < hi || end >= 0x7fffffffLL;
    hipLaunchKernelGGL(rd_bam_find_init_kernel, dim3(1), dim3(1), 0, st, (unsigned long long *)info, bad ? 1 : 0);
    if (!bad && hi > lo) {
        const int64_t grid = (hi - lo + BAM_FIND_CAND - 1) / BAM_FIND_CAND;      // (< 2^19)
        hipLaunchKernelGGL(rd_bam_find_kernel, dim3((unsigned)grid), dim3(BAM_FIND_THREADS), 0, st, text, lo, hi, end, (int)at_eof, (unsigned long long *)info);
    }
    RD_HIP(hipGetLastError());
    return RD_OK;
}

size_t rd_bam_count_workspace_bytes(int64_t text_end) {
    if (text_end < 0 || text_end >= 0x7fffffffLL) return 0;
    return bam_count_ws(nullptr, text_end).total;
}

int rd_bam_count(uint8_t *text, int64_t pad, int64_t end, const uint8_t *prev_text, const rd_fq_summary *prev, int32_t final, rd_fq_summary *summary, void *workspace,
                 size_t workspace_bytes, void *stream) {
    if (const int rc = fq_index_check("rd_bam_count", text, pad, end, prev_text, prev, (const int32_t *)text, 0, summary, workspace, false, false, nullptr)) return rc;
    const BamCountWs p = bam_count_ws(workspace, end);
    if (workspace_bytes < p.total) RD_FAIL(RD_E_WORKSPACE, "rd_bam_count: workspace too small: %zu < %zu", workspace_bytes, p.total);
    hipStream_t st = (hipStream_t)stream;
    FqSummary *sum = (FqSummary *)summary;
    hipLaunchKernelGGL(rd_fq_begin_kernel<false>, dim3(1), dim3(FQ_THREADS), 0, st, text, pad, end, prev_text, (const FqSummary *)prev, (int)final, sum);
    hipLaunchKernelGGL(rd_bam_walk_kernel<false>, dim3(p.nseg), dim3(64), 0, st, text, sum, p.seg, (int2 *)nullptr);
    hipLaunchKernelGGL(rd_bam_stitch_kernel<false>, dim3(1), dim3(64), 0, st, text, sum, p.seg, (int2 *)nullptr, p.nseg, (int32_t *)nullptr, (int64_t *)nullptr,
                       (int32_t *)nullptr, (BamScratch *)nullptr, (int)final, (int64_t)0, (int64_t)0, (int64_t *)nullptr);
    RD_HIP(hipGetLastError());
    return RD_OK;
}

// ---- the delivered BAM records as they stand in the input (rd_bam_raw.hpp): the source offsets rd_bam_index left in its workspace
int32_t *rd_bam_index_src(void *workspace, int64_t text_end) {
    if (!workspace || text_end < 0 || text_end >= 0x7fffffffLL) return nullptr;
    return bam_ws(workspace, text_end).src_tab;
}

int rd_bam_raw_tab(const uint8_t *text, const int32_t *src_tab, const rd_fq_summary *summary, int64_t *raw_tab, int64_t cap_records, int64_t every, int32_t *samples,
                   int64_t cap_samples, void *stream) {
    if (!text || !src_tab || !summary || !raw_tab || (cap_samples > 0 && !samples)) RD_FAIL(RD_E_INVALID, "rd_bam_raw_tab: null pointer");
    if (cap_records < 1 || cap_records > 0x7fffffffLL || every < 1 || cap_samples < 0) RD_FAIL(RD_E_INVALID, "rd_bam_raw_tab: bad cap_records / every / cap_samples");
    hipStream_t st = (hipStream_t)stream;
    const FqSummary *sum = (const FqSummary *)summary;
    const unsigned nb = (unsigned)((cap_records + GZ_SCAN_ITEMS - 1) / GZ_SCAN_ITEMS);
    hipLaunchKernelGGL(rd_bam_raw_local_kernel, dim3(nb), dim3(256), 0, st, text, src_tab, sum, raw_tab, cap_records);
    hipLaunchKernelGGL(rd_bam_raw_base_kernel, dim3(1), dim3(256), 0, st, sum, raw_tab);
    hipLaunchKernelGGL(rd_bam_raw_add_kernel, dim3(nb), dim3(256), 0, st, sum, raw_tab);
    if (cap_samples > 0) {
        int64_t grid = cap_samples / FQ_THREADS + 1;
        if (grid > 1024) grid = 1024;
        hipLaunchKernelGGL(rd_bam_raw_sample_kernel, dim3((unsigned)grid), dim3(FQ_THREADS), 0, st, (const int64_t *)raw_tab, sum, every, samples, cap_samples);
    }
    RD_HIP(hipGetLastError());
    return RD_OK;
}

int rd_bam_raw_gather(const uint8_t *text, const int32_t *src_tab, const int64_t *raw_tab, const rd_fq_summary *summary, int64_t rec_lo, int64_t rec_hi,
                      int64_t max_bytes, uint8_t *out, int64_t out_cap, const int64_t *cursor_in, int64_t *cursor_out, int64_t *raw_start, void *stream) {
    if (!text || !src_tab || !raw_tab || !summary || !out || !cursor_in || !cursor_out || !raw_start) RD_FAIL(RD_E_INVALID, "rd_bam_raw_gather: null pointer");
    if (rec_lo < 0 || rec_hi < rec_lo || max_bytes < 0 || out_cap < 0 || cursor_in == cursor_out) RD_FAIL(RD_E_INVALID, "rd_bam_raw_gather: bad range");
    if ((uintptr_t)out & 15) RD_FAIL(RD_E_INVALID, "rd_bam_raw_gather: out must be 16-byte aligned");
    int64_t grid = max_bytes / (BAM_RAW_BYTES * 4) + 1;         // four 16-byte granules per thread
    const int64_t grid_r = (rec_hi - rec_lo) / FQ_THREADS + 1;
    if (grid < grid_r) grid = grid_r;
    if (grid > 8192) grid = 8192;
    hipLaunchKernelGGL(rd_bam_raw_gather_kernel, dim3((unsigned)grid), dim3(FQ_THREADS), 0, (hipStream_t)stream, text, src_tab, raw_tab, (const FqSummary *)summary, rec_lo,
                       rec_hi, out, out_cap, cursor_in, cursor_out, raw_start);
    RD_HIP(hipGetLastError());
    return RD_OK;
}

// the per-read report of a chunk (rd_report.hpp): one line per record, and the lines' starts as a record table of the report text
namespace {
struct ReportWs {
    int nb;
    int32_t *idlen, *fault;
    uint64_t *qs;
    int64_t *bsum;
    size_t total;
};
ReportWs report_ws(void *workspace, int64_t n) {
    ReportWs p;
    Carver c(workspace);
    p.nb = scan_blocks(n);
    p.idlen = c.take<int32_t>((size_t)n);
    p.qs = c.take<uint64_t>((size_t)n);
    p.bsum = c.take<int64_t>((size_t)p.nb);
    p.fault = c.take<int32_t>(1);
    p.total = c.off;
    return p;
}
}  // namespace

size_t rd_report_workspace_bytes(int64_t n) {
    if (n < 0) return 0;
    return report_ws(nullptr, n).total;
}

size_t rd_report_out_bound(int64_t n, int64_t text_bytes) {
    if (n < 0 || text_bytes < 0) return 0;
    return (size_t)text_bytes + (size_t)n * RP_MAX_SUFFIX;      // an id is shorter than its record
}

int rd_report_format(const uint8_t *text, int64_t text_bytes, const int64_t *rec_start, int64_t n, const float *logits_a, const float *logits_b,
                     const int8_t *labels, uint8_t *out, size_t out_cap, int64_t *line_start, int64_t *info, void *workspace, size_t workspace_bytes,
                     void *stream) {
    if (n < 0 || n > 0x7fffffffLL || text_bytes < 0) RD_FAIL(RD_E_INVALID, "rd_report_format: bad n or text_bytes");
    if (!info || !line_start) RD_FAIL(RD_E_INVALID, "rd_report_format: null info or line_start");
    hipStream_t st = (hipStream_t)stream;
    if (n == 0) {
        RD_HIP(hipMemsetAsync(info, 0, 4 * sizeof(int64_t), st));
        RD_HIP(hipMemsetAsync(line_start, 0, sizeof(int64_t), st));
        return RD_OK;
    }
    if ((!text && text_bytes > 0) || !rec_start || !logits_a || !labels || !out || !workspace) RD_FAIL(RD_E_INVALID, "rd_report_format: null pointer");
    if (((uintptr_t)workspace & 255) || ((uintptr_t)out & 15)) RD_FAIL(RD_E_INVALID, "rd_report_format: workspace must be 256-byte aligned, out 16-byte aligned");
    const ReportWs p = report_ws(workspace, n);
    if (workspace_bytes < p.total) RD_FAIL(RD_E_WORKSPACE, "rd_report_format: workspace too small: %zu < %zu", workspace_bytes, p.total);
    RD_HIP(hipMemsetAsync(p.fault, 0, sizeof(int32_t), st));
    hipLaunchKernelGGL(rd_report_len_kernel, dim3(p.nb), dim3(256), 0, st, text, text_bytes, rec_start, n, logits_a, logits_b, labels, line_start, p.idlen, p.qs, p.bsum, p.fault);
    scan_base(p.bsum, p.nb, info, (int64_t)(out_cap < (size_t)INT64_MAX ? out_cap : (size_t)INT64_MAX), st);
    hipLaunchKernelGGL((rd_scan_off_kernel<8, 1, ScanTab<1>, RpVerdict>), dim3(p.nb), dim3(256), 0, st, ScanTab<1>{{line_start}}, n, ScanOut<1>{{line_start}, {p.bsum}},
                       RpVerdict{n, p.fault, info});
    hipLaunchKernelGGL(rd_report_write_kernel, dim3((unsigned)((n + RP_LINES - 1) / RP_LINES)), dim3(256), 0, st, text, rec_start, line_start, n, p.idlen, p.qs, labels,
                       logits_b ? 3 : 1, out, info);
    RD_HIP(hipGetLastError());
    return RD_OK;
}

// paired-end reads from one interleaved chunk (rd_pairs.hpp): no workspace, one pass over the tables
int rd_pair_split(const uint8_t *text, int64_t text_bytes, const int64_t *rec_start, const int64_t *seq_off, const int32_t *seq_len, int64_t n_pairs,
                  int32_t check_ids, int64_t *pair_start, int64_t *seq_off1, int32_t *seq_len1, int64_t *seq_off2, int32_t *seq_len2, int64_t *info,
                  void *stream) {
    if (n_pairs < 0 || n_pairs > 0x3fffffffLL || text_bytes < 0) RD_FAIL(RD_E_INVALID, "rd_pair_split: bad n_pairs or text_bytes");
    if (!info || !rec_start || !pair_start) RD_FAIL(RD_E_INVALID, "rd_pair_split: null info, rec_start or pair_start");
    if (n_pairs > 0 && ((!text && text_bytes > 0) || !seq_off || !seq_len || !seq_off1 || !seq_len1 || !seq_off2 || !seq_len2))
        RD_FAIL(RD_E_INVALID, "rd_pair_split: null pointer");
    hipStream_t st = (hipStream_t)stream;
    RD_HIP(hipMemsetAsync(info, 0, 4 * sizeof(int64_t), st));
    RD_HIP(hipMemsetAsync(info + 1, 0xff, sizeof(int64_t), st));      // -1: no pair failed the mate check (the kernel takes an unsigned minimum)
    hipLaunchKernelGGL(rd_pair_split_kernel, dim3((unsigned)((n_pairs + 256 * PS_PAIRS) / (256 * PS_PAIRS))), dim3(256), 0, st, text, text_bytes, rec_start,
                       seq_off, seq_len, n_pairs, (int)(check_ids != 0), pair_start, seq_off1, seq_len1, seq_off2, seq_len2, info);
    RD_HIP(hipGetLastError());
    return RD_OK;
}

int rd_pair_expand_labels(const int8_t *pair_labels, int64_t n_pairs, int32_t mate, int8_t *rec_labels, void *stream) {
    if (n_pairs < 0 || n_pairs > 0x3fffffffLL) RD_FAIL(RD_E_INVALID, "rd_pair_expand_labels: bad n_pairs");
    if (mate != 0 && mate != 1) RD_FAIL(RD_E_INVALID, "rd_pair_expand_labels: mate must be 0 or 1; got %d", mate);
    if (n_pairs == 0) return RD_OK;
    if (!pair_labels || !rec_labels) RD_FAIL(RD_E_INVALID, "rd_pair_expand_labels: null pointer");
    hipLaunchKernelGGL(rd_pair_expand_kernel, dim3((unsigned)((n_pairs + 2047) / 2048)), dim3(256), 0, (hipStream_t)stream, pair_labels, n_pairs, (int)mate, rec_labels);
    RD_HIP(hipGetLastError());
    return RD_OK;
}

// the QC counters of a run (rd_summary.hpp): acc += the counters of this chunk, or nothing when the check pass finds a bad entry
int64_t rd_summary_words(void) { return RD_SUM_WORDS; }

int rd_summary_accumulate(const uint8_t *text_a, int64_t bytes_a, const int64_t *seq_off_a, const int32_t *seq_len_a, const float *logits_a,
                          const uint8_t *text_b, int64_t bytes_b, const int64_t *seq_off_b, const int32_t *seq_len_b, const float *logits_b,
                          const int8_t *labels, int64_t n, int64_t *acc, int64_t *info, void *stream) {
    if (n < 0 || n > 0x7fffffffLL || bytes_a < 0 || bytes_b < 0) RD_FAIL(RD_E_INVALID, "rd_summary_accumulate: bad n or text bytes");
    hipStream_t st = (hipStream_t)stream;
    if (n == 0) {
        if (info) RD_HIP(hipMemsetAsync(info, 0, 4 * sizeof(int64_t), st));
        return RD_OK;
    }
    if (!acc || !info || !labels || (!text_a && bytes_a > 0) || !seq_off_a || !seq_len_a || !logits_a) RD_FAIL(RD_E_INVALID, "rd_summary_accumulate: null pointer");
    if (text_b && (!seq_off_b || !seq_len_b || !logits_b)) RD_FAIL(RD_E_INVALID, "rd_summary_accumulate: mate 2 needs its tables and logits");
    if (!text_b) seq_off_b = nullptr;                     // (single-end: the check pass skips mate 2 by this pointer)
    RD_HIP(hipMemsetAsync(info, 0, 4 * sizeof(int64_t), st));
    hipLaunchKernelGGL(rd_summary_check_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, bytes_a, seq_off_a, seq_len_a, bytes_b, seq_off_b, seq_len_b,
                       labels, n, info);
    hipLaunchKernelGGL(rd_summary_acc_kernel, dim3((unsigned)((n + SM_UNITS - 1) / SM_UNITS)), dim3(256), 0, st, text_a, seq_off_a, seq_len_a, logits_a, text_b,
                       seq_off_b, seq_len_b, logits_b, labels, n, acc, info);
    RD_HIP(hipGetLastError());
    return RD_OK;
}

// the optional fields of the raw BAM records of a chunk (rd_bam_tags.hpp): where a tag's value lies, which declared read group it names,
// and the units and bases per (group, class)
namespace {
// lanes per record of rd_bam_tag_find: 4 for short records, 16 when a record's mean size says that long Z / B values are the rule
// (DESIGN.md §3.23 has the measurement, also of 1 and 64 lanes, which lost on both shapes); RD_TAG_LANES = 4 / 16 overrides it, so that
// tools/groups_bench.py can time each mapping on each shape
int tag_lanes(int64_t raw_bytes, int64_t n_rec) {
    if (const char *e = getenv("RD_TAG_LANES")) {
        const int v = atoi(e);
        if (v == 4 || v == 16) return v;
    }
    return raw_bytes / n_rec >= 1024 ? 16 : 4;
}
}  // namespace

int rd_bam_tag_find(const uint8_t *raw, int64_t raw_bytes, const int64_t *raw_start, int64_t n_rec, const uint8_t *tag, int64_t *val_off, int32_t *val_len,
                    uint8_t *val_type, void *stream) {
    if (n_rec < 0 || n_rec > 0x7fffffffLL / 64 || raw_bytes < 0) RD_FAIL(RD_E_INVALID, "rd_bam_tag_find: bad n_rec or raw_bytes");
    if (!tag) RD_FAIL(RD_E_INVALID, "rd_bam_tag_find: null pointer");
    if (n_rec == 0) return RD_OK;
    if ((!raw && raw_bytes > 0) || !raw_start || !val_off || !val_len || !val_type) RD_FAIL(RD_E_INVALID, "rd_bam_tag_find: null pointer");
    const uint32_t want = (uint32_t)tag[0] | ((uint32_t)tag[1] << 8);
    hipStream_t st = (hipStream_t)stream;
    if (tag_lanes(raw_bytes, n_rec) == 16) tag_find_launch<16>(raw, raw_bytes, raw_start, n_rec, want, val_off, val_len, val_type, st);
    else tag_find_launch<4>(raw, raw_bytes, raw_start, n_rec, want, val_off, val_len, val_type, st);
    RD_HIP(hipGetLastError());
    return RD_OK;
}

int rd_bam_group_rows(const uint8_t *raw, const int64_t *val_off, const int32_t *val_len, const uint8_t *val_type, int64_t n_rec, const uint8_t *dict_bytes,
                      const int32_t *dict_off, int32_t G, int32_t *rows, void *stream) {
    if (n_rec < 0 || n_rec > 0x7fffffffLL || G < 0 || G > RD_GROUPS_MAX) RD_FAIL(RD_E_INVALID, "rd_bam_group_rows: bad n_rec or G");
    if (n_rec == 0) return RD_OK;
    if (!raw || !val_off || !val_len || !val_type || !rows || !dict_off || (G > 0 && !dict_bytes)) RD_FAIL(RD_E_INVALID, "rd_bam_group_rows: null pointer");
    const int64_t wgs = (n_rec + GR_THREADS - 1) / GR_THREADS;
    if (G <= GR_ROWS_LDS)                                 // the dictionary in LDS, staged once per workgroup: fewer, longer-lived workgroups
        hipLaunchKernelGGL(rd_bam_group_rows_lds_kernel, dim3((unsigned)(wgs < 1024 ? wgs : 1024)), dim3(GR_THREADS), 0, (hipStream_t)stream, raw, val_off, val_len,
                           val_type, n_rec, dict_bytes, dict_off, G, rows);
    else
        hipLaunchKernelGGL(rd_bam_group_rows_kernel, dim3((unsigned)wgs), dim3(GR_THREADS), 0, (hipStream_t)stream, raw, val_off, val_len, val_type, n_rec, dict_bytes,
                           dict_off, G, rows);
    RD_HIP(hipGetLastError());
    return RD_OK;
}

int rd_bam_group_accumulate(const uint8_t *raw_a, const int64_t *raw_start_a, const int32_t *rows_a, int64_t first_a, int64_t stride_a, const uint8_t *raw_b,
                            const int64_t *raw_start_b, const int32_t *rows_b, int64_t first_b, int64_t stride_b, const int8_t *labels, int64_t n, int32_t G,
                            int64_t *acc, int64_t *info, void *stream) {
    if (n < 0 || n > 0x7fffffffLL || G < 0 || G > RD_GROUPS_MAX) RD_FAIL(RD_E_INVALID, "rd_bam_group_accumulate: bad n or G");
    if (first_a < 0 || stride_a < 1 || (raw_b && (first_b < 0 || stride_b < 1))) RD_FAIL(RD_E_INVALID, "rd_bam_group_accumulate: bad first / stride");
    hipStream_t st = (hipStream_t)stream;
    if (n == 0) {
        if (info) RD_HIP(hipMemsetAsync(info, 0, 4 * sizeof(int64_t), st));
        return RD_OK;
    }
    if (!acc || !info || !labels || !raw_a || !raw_start_a || !rows_a) RD_FAIL(RD_E_INVALID, "rd_bam_group_accumulate: null pointer");
    if (raw_b && (!raw_start_b || !rows_b)) RD_FAIL(RD_E_INVALID, "rd_bam_group_accumulate: mate 2 needs its record table and rows");
    if (!raw_b) rows_b = nullptr;                         // (single-end: the check pass skips mate 2 by this pointer)
    RD_HIP(hipMemsetAsync(info, 0, 4 * sizeof(int64_t), st));
    hipLaunchKernelGGL(rd_bam_group_check_kernel, dim3((unsigned)((n + GR_THREADS - 1) / GR_THREADS)), dim3(GR_THREADS), 0, st, rows_a, first_a, stride_a, rows_b, first_b,
                       stride_b, labels, n, G, info);
    const int64_t tiles = (n + GR_THREADS - 1) / GR_THREADS;
    hipLaunchKernelGGL(rd_bam_group_acc_kernel, dim3((unsigned)(tiles < GR_MAX_WGS ? tiles : GR_MAX_WGS)), dim3(GR_THREADS), 0, st, raw_a, raw_start_a, rows_a, first_a,
                       stride_a, raw_b, raw_start_b, rows_b, first_b, stride_b, labels, n, G, acc, info);
    RD_HIP(hipGetLastError());
    return RD_OK;
}

// the listed tags of a chunk's raw records as text behind the read names of its FASTQ text (rd_bam_tagtext.hpp): one walk per listed tag
// (rd_bam_tag_find's kernel, into tables of the workspace), the count pass, the scan into out_start, the write pass
namespace {
TagTextWs tagtext_ws(void *workspace, int64_t n, int32_t n_tags) {
    TagTextWs p;
    Carver c(workspace);
    const size_t cells = (size_t)n * (size_t)n_tags;
    p.nb = scan_blocks(n);
    p.val_off = c.take<int64_t>(cells);
    p.val_len = c.take<int32_t>(cells);
    p.val_type = c.take<uint8_t>(cells);
    p.tag_bytes = c.take<int64_t>(cells);
    p.hdr = c.take<int64_t>((size_t)n);
    p.flags = c.take<uint8_t>((size_t)n);
    p.bsum = c.take<int64_t>((size_t)p.nb);
    p.tot = c.take<int64_t>(4);
    p.cnt = c.take<unsigned long long>(TT_CNT);
    p.fault = c.take<int32_t>(1);
    p.total = c.off;
    return p;
}
bool tag_name_ok(const uint8_t *t) {
    const bool a = (t[0] >= 'A' && t[0] <= 'Z') || (t[0] >= 'a' && t[0] <= 'z');
    return a && ((t[1] >= 'A' && t[1] <= 'Z') || (t[1] >= 'a' && t[1] <= 'z') || (t[1] >= '0' && t[1] <= '9'));
}
}  // namespace

size_t rd_bam_tag_splice_workspace_bytes(int64_t n_rec, int32_t n_tags) {
    if (n_rec < 0 || n_rec > 0x7fffffffLL / 64 || n_tags < 1 || n_tags > RD_BAM_TAGS_MAX) return 0;
    return tagtext_ws(nullptr, n_rec, n_tags).total;
}

int rd_bam_tag_splice(const uint8_t *text, int64_t text_bytes, const int64_t *rec_start, const uint8_t *raw, int64_t raw_bytes, const int64_t *raw_start,
                      int64_t n_rec, const uint8_t *tags, int32_t n_tags, uint8_t *out, size_t out_cap, int64_t *out_start, int64_t *info, void *workspace,
                      size_t workspace_bytes, void *stream) {
    return rd_bam_tag_splice_ex(text, text_bytes, rec_start, raw, raw_bytes, raw_start, n_rec, tags, n_tags, out, out_cap, out_start, info, workspace, workspace_bytes, 0u,
                                stream);
}

// flags & RD_BAM_TAGS_FLOATS: the count and the write pass that format f and B:f values (rd_float_text.hpp); the tables and the
// workspace are the same
int rd_bam_tag_splice_ex(const uint8_t *text, int64_t text_bytes, const int64_t *rec_start, const uint8_t *raw, int64_t raw_bytes, const int64_t *raw_start,
                         int64_t n_rec, const uint8_t *tags, int32_t n_tags, uint8_t *out, size_t out_cap, int64_t *out_start, int64_t *info, void *workspace,
                         size_t workspace_bytes, uint32_t flags, void *stream) {
    if (flags & ~RD_BAM_TAGS_FLOATS) RD_FAIL(RD_E_INVALID, "rd_bam_tag_splice: unknown flag bits 0x%x", flags & ~RD_BAM_TAGS_FLOATS);
    const bool floats = (flags & RD_BAM_TAGS_FLOATS) != 0;
    if (n_rec < 0 || n_rec > 0x7fffffffLL / 64 || text_bytes < 0 || raw_bytes < 0) RD_FAIL(RD_E_INVALID, "rd_bam_tag_splice: bad n_rec, text_bytes or raw_bytes");
    if (n_tags < 1 || n_tags > RD_BAM_TAGS_MAX) RD_FAIL(RD_E_INVALID, "rd_bam_tag_splice: n_tags=%d out of range [1,%d]", n_tags, RD_BAM_TAGS_MAX);
    if (!tags) RD_FAIL(RD_E_INVALID, "rd_bam_tag_splice: null pointer");
    TtNames names;
    memset(&names, 0, sizeof(names));
    for (int j = 0; j < n_tags; ++j) {
        if (!tag_name_ok(tags + 2 * j)) RD_FAIL(RD_E_INVALID, "rd_bam_tag_splice: tag %d is not a name ([A-Za-z][A-Za-z0-9])", j);
        for (int i = 0; i < j; ++i)
            if (tags[2 * i] == tags[2 * j] && tags[2 * i + 1] == tags[2 * j + 1]) RD_FAIL(RD_E_INVALID, "rd_bam_tag_splice: tag %d appears twice", j);
        names.b[2 * j] = tags[2 * j];
        names.b[2 * j + 1] = tags[2 * j + 1];
    }
    if (!info) RD_FAIL(RD_E_INVALID, "rd_bam_tag_splice: null info");
    hipStream_t st = (hipStream_t)stream;
    if (n_rec == 0) {
        RD_HIP(hipMemsetAsync(info, 0, (8 + RD_BAM_TAGS_MAX) * sizeof(int64_t), st));
        return RD_OK;
    }
    if (!text || !rec_start || !raw_start || (!raw && raw_bytes > 0) || !out || !out_start || !workspace) RD_FAIL(RD_E_INVALID, "rd_bam_tag_splice: null pointer");
    if (((uintptr_t)workspace & 255) || ((uintptr_t)out & 15)) RD_FAIL(RD_E_INVALID, "rd_bam_tag_splice: workspace must be 256-byte aligned, out 16-byte aligned");
    const TagTextWs p = tagtext_ws(workspace, n_rec, n_tags);
    if (workspace_bytes < p.total) RD_FAIL(RD_E_WORKSPACE, "rd_bam_tag_splice: workspace too small: %zu < %zu", workspace_bytes, p.total);
    const int64_t cap = (int64_t)(out_cap < (size_t)INT64_MAX ? out_cap : (size_t)INT64_MAX);
    RD_HIP(hipMemsetAsync(p.cnt, 0, (size_t)((char *)p.fault - (char *)p.cnt) + sizeof(int32_t), st));      // (the counters and the fault word)
    const bool wide = tag_lanes(raw_bytes, n_rec) == 16;
    if (wide && floats)
        tagtext_launch<16, true>(text, text_bytes, rec_start, raw, raw_bytes, raw_start, n_rec, n_tags, names, out, cap, out_start, info, p, st);
    else if (wide)
        tagtext_launch<16, false>(text, text_bytes, rec_start, raw, raw_bytes, raw_start, n_rec, n_tags, names, out, cap, out_start, info, p, st);
    else if (floats)
        tagtext_launch<4, true>(text, text_bytes, rec_start, raw, raw_bytes, raw_start, n_rec, n_tags, names, out, cap, out_start, info, p, st);
    else
        tagtext_launch<4, false>(text, text_bytes, rec_start, raw, raw_bytes, raw_start, n_rec, n_tags, names, out, cap, out_start, info, p, st);
    RD_HIP(hipGetLastError());
    return RD_OK;
}

// the records of a FASTQ / FASTA chunk as unaligned BAM records (rd_bam_encode.hpp): lengths, their scan, the write pass by output tiles
namespace {
BamEncodeWs bam_encode_ws(void *workspace, int64_t n, int32_t n_names = 0) {
    BamEncodeWs p;
    Carver c(workspace);
    p.nb = scan_blocks(n);
    p.meta = c.take<uint32_t>((size_t)n);
    p.qoff = c.take<int64_t>((size_t)n);
    p.bsum = c.take<int64_t>((size_t)p.nb);
    p.first_bad = c.take<unsigned long long>(2);
    p.starred = c.take<unsigned long long>(1);
    p.fault = c.take<int32_t>(1);
    p.tagb = p.foff = p.fend = p.ooff = p.tot = nullptr;
    p.mask = nullptr;
    p.cnt = nullptr;
    if (n_names > 0) {
        const size_t cells = (size_t)n * (size_t)n_names;
        p.tagb = c.take<int64_t>((size_t)n);
        p.foff = c.take<int64_t>(cells);
        p.fend = c.take<int64_t>(cells);
        p.ooff = c.take<int64_t>(cells);
        p.tot = c.take<int64_t>(4);
        p.mask = c.take<uint32_t>((size_t)n);
        p.cnt = c.take<unsigned long long>(BT_CNT);
    }
    p.total = c.off;
    return p;
}

}  // namespace

size_t rd_bam_encode_workspace_bytes(int64_t n_rec) {
    if (n_rec < 0 || n_rec > 0x3fffffffLL) return 0;
    return bam_encode_ws(nullptr, n_rec).total;
}

size_t rd_bam_encode_tags_workspace_bytes(int64_t n_rec, int32_t n_names) {
    if (n_rec < 0 || n_rec > 0x3fffffffLL || n_names < 0 || n_names > RD_BAM_TAGS_MAX) return 0;
    return bam_encode_ws(nullptr, n_rec, n_names).total;
}

int rd_bam_encode(const uint8_t *text, int64_t text_bytes, const int64_t *rec_start, const int64_t *seq_off, const int32_t *seq_len, int64_t n_rec, int64_t rec_first,
                  int32_t rec_stride, uint32_t flags, uint8_t *raw, size_t raw_cap, int64_t *raw_start, int64_t *info, void *workspace, size_t workspace_bytes,
                  void *stream) {
    return rd_bam_encode_ex(text, text_bytes, rec_start, seq_off, seq_len, n_rec, rec_first, rec_stride, flags, nullptr, 0, raw, raw_cap, raw_start, info, workspace,
                            workspace_bytes, stream);
}

// n_names == 0: the launches of rd_bam_encode (the kernels' TAGS = false instances). Else the tag count pass in front of the length pass
// (whose lengths include the tags' bytes), the scan without a limit - the verdict holds the total against raw_cap and reports it -, the
// tile writer and the tag pass behind it
int rd_bam_encode_ex(const uint8_t *text, int64_t text_bytes, const int64_t *rec_start, const int64_t *seq_off, const int32_t *seq_len, int64_t n_rec, int64_t rec_first,
                     int32_t rec_stride, uint32_t flags, const uint8_t *names, int32_t n_names, uint8_t *raw, size_t raw_cap, int64_t *raw_start, int64_t *info,
                     void *workspace, size_t workspace_bytes, void *stream) {
    const char *fn = n_names ? "rd_bam_encode_ex" : "rd_bam_encode";
    const uint32_t known = RD_UBAM_FASTA | (0xfffu << RD_UBAM_EVEN_SHIFT) | (0xfffu << RD_UBAM_ODD_SHIFT) | (n_names > 0 ? RD_UBAM_TAG_FLOATS : 0u);
    if (flags & ~known & RD_UBAM_TAG_FLOATS) RD_FAIL(RD_E_INVALID, "%s: RD_UBAM_TAG_FLOATS without listed names", fn);
    if (flags & ~known) RD_FAIL(RD_E_INVALID, "%s: unknown flag bits 0x%x", fn, flags & ~known);
    if (n_rec < 0 || n_rec > 0x3fffffffLL || text_bytes < 0) RD_FAIL(RD_E_INVALID, "%s: bad n_rec or text_bytes", fn);
    if (rec_first < 0 || rec_stride < 1 || rec_first > 0x3fffffffLL) RD_FAIL(RD_E_INVALID, "%s: bad rec_first or rec_stride", fn);
    if (n_names < 0 || n_names > RD_BAM_TAGS_MAX) RD_FAIL(RD_E_INVALID, "rd_bam_encode_ex: n_names=%d out of range [0,%d]", n_names, RD_BAM_TAGS_MAX);
    if (n_names && !names) RD_FAIL(RD_E_INVALID, "rd_bam_encode_ex: null names");
    TtNames nm;
    memset(&nm, 0, sizeof(nm));
    for (int j = 0; j < n_names; ++j) {
        if (!tag_name_ok(names + 2 * j)) RD_FAIL(RD_E_INVALID, "rd_bam_encode_ex: name %d is not a tag name ([A-Za-z][A-Za-z0-9])", j);
        for (int i = 0; i < j; ++i)
            if (names[2 * i] == names[2 * j] && names[2 * i + 1] == names[2 * j + 1]) RD_FAIL(RD_E_INVALID, "rd_bam_encode_ex: name %d appears twice", j);
        nm.b[2 * j] = names[2 * j];
        nm.b[2 * j + 1] = names[2 * j + 1];
    }
    if (!info || !raw_start) RD_FAIL(RD_E_INVALID, "%s: null info or raw_start", fn);
    hipStream_t st = (hipStream_t)stream;
    RD_HIP(hipMemsetAsync(info, 0, (size_t)(n_names ? 10 + n_names : 8) * sizeof(int64_t), st));
    if (n_rec == 0) {
        RD_HIP(hipMemsetAsync(info + 2, 0xff, sizeof(int64_t), st));
        RD_HIP(hipMemsetAsync(info + 7, 0xff, sizeof(int64_t), st));
        RD_HIP(hipMemsetAsync(raw_start, 0, sizeof(int64_t), st));
        return RD_OK;
    }
    if ((!text && text_bytes > 0) || !rec_start || !seq_off || !seq_len || !raw || !workspace) RD_FAIL(RD_E_INVALID, "%s: null pointer", fn);
    if (((uintptr_t)workspace & 255) || ((uintptr_t)raw & 15)) RD_FAIL(RD_E_INVALID, "%s: workspace must be 256-byte aligned, raw 16-byte aligned", fn);
    const BamEncodeWs p = bam_encode_ws(workspace, n_rec, n_names);
    if (workspace_bytes < p.total) RD_FAIL(RD_E_WORKSPACE, "%s: workspace too small: %zu < %zu", fn, workspace_bytes, p.total);
    const int64_t cap = (int64_t)(raw_cap < (size_t)INT64_MAX ? raw_cap : (size_t)INT64_MAX);
    RD_HIP(hipMemsetAsync(p.first_bad, 0xff, 2 * sizeof(unsigned long long), st));
    RD_HIP(hipMemsetAsync(p.starred, 0, (size_t)((char *)p.fault - (char *)p.starred) + sizeof(int32_t), st));
    const BeTabs t = {rec_start, seq_off, seq_len, rec_first, rec_stride};
    // the tiles of the bound - or of raw_cap when that is less: the bytes are known on the device only, the workgroups stride over them.
    // (Tags take at most twice their text: rd_bam_encode.hpp.)
    const int64_t fq = text_bytes + 32 * n_rec, fa = text_bytes + (text_bytes + 1) / 2 + 40 * n_rec;
    int64_t most = flags & RD_UBAM_FASTA ? fa : fq;
    if (n_names) most += 2 * text_bytes;
    if (most > cap) most = cap;
    int64_t grid = (most + BE_TILE - 1) / BE_TILE;
    if (grid < 1) grid = 1;
    if (grid > BE_GRID) grid = BE_GRID;
    if (n_names) {
        RD_HIP(hipMemsetAsync(p.cnt, 0, BT_CNT * sizeof(unsigned long long), st));
        const bool wide = tag_lanes(text_bytes, n_rec) == 16, floats = flags & RD_UBAM_TAG_FLOATS;
        if (wide && floats) bam_encode_tags_launch<16, true>(text, text_bytes, t, n_rec, flags, nm, n_names, raw, cap, raw_start, info, p, (unsigned)grid, st);
        else if (wide) bam_encode_tags_launch<16, false>(text, text_bytes, t, n_rec, flags, nm, n_names, raw, cap, raw_start, info, p, (unsigned)grid, st);
        else if (floats) bam_encode_tags_launch<4, true>(text, text_bytes, t, n_rec, flags, nm, n_names, raw, cap, raw_start, info, p, (unsigned)grid, st);
        else bam_encode_tags_launch<4, false>(text, text_bytes, t, n_rec, flags, nm, n_names, raw, cap, raw_start, info, p, (unsigned)grid, st);
        RD_HIP(hipGetLastError());
        return RD_OK;
    }
    hipLaunchKernelGGL(rd_be_len_kernel<false>, dim3(p.nb), dim3(256), 0, st, text, text_bytes, t, n_rec, flags, raw_start, p.meta, p.qoff, p.bsum, p.first_bad, p.fault,
                       p.starred, (const int64_t *)nullptr);
    scan_base(p.bsum, p.nb, info, cap, st);
    hipLaunchKernelGGL((rd_scan_off_kernel<8, 1, ScanTab<1>, BeVerdict>), dim3(p.nb), dim3(256), 0, st, ScanTab<1>{{raw_start}}, n_rec, ScanOut<1>{{raw_start}, {p.bsum}},
                       BeVerdict{n_rec, p.fault, p.first_bad, p.starred, info});
    hipLaunchKernelGGL(rd_be_write_kernel<false>, dim3((unsigned)grid), dim3(256), 0, st, text, t, n_rec, flags, (const uint32_t *)p.meta, (const int64_t *)p.qoff,
                       raw_start, raw, info, (const int64_t *)nullptr);
    RD_HIP(hipGetLastError());
    return RD_OK;
}

// float32 bit patterns as their %g text (rd_float_text.hpp), one 16-byte slot and one length per value
int rd_float_text(const uint32_t *bits, int64_t n, uint8_t *text, uint8_t *len, void *stream) {
    if (n < 0) RD_FAIL(RD_E_INVALID, "rd_float_text: n=%lld is negative", (long long)n);
    if (n == 0) return RD_OK;
    if (!bits || !text || !len) RD_FAIL(RD_E_INVALID, "rd_float_text: null pointer");
    if (((uintptr_t)bits & 3) || ((uintptr_t)text & 15)) RD_FAIL(RD_E_INVALID, "rd_float_text: bits must be 4-byte aligned, text 16-byte aligned");
    const int64_t wgs = (n + FT_THREADS - 1) / FT_THREADS;
    hipLaunchKernelGGL(rd_float_text_kernel, dim3((unsigned)(wgs < FT_MAX_WGS ? wgs : FT_MAX_WGS)), dim3(FT_THREADS), 0, (hipStream_t)stream, bits, n, text, len);
    RD_HIP(hipGetLastError());
    return RD_OK;
}

// the text of float values as the nearest float32 (rd_float_parse.hpp), one lane per value
int rd_float_parse(const uint8_t *text, const int64_t *start, int64_t n, uint32_t *bits, uint8_t *status, void *stream) {
    if (n < 0) RD_FAIL(RD_E_INVALID, "rd_float_parse: n=%lld is negative", (long long)n);
    if (n == 0) return RD_OK;
    if (!text || !start || !bits || !status) RD_FAIL(RD_E_INVALID, "rd_float_parse: null pointer");
    if (((uintptr_t)start & 7) || ((uintptr_t)bits & 3)) RD_FAIL(RD_E_INVALID, "rd_float_parse: start must be 8-byte aligned, bits 4-byte aligned");
    const int64_t wgs = (n + FP_THREADS - 1) / FP_THREADS;
    hipLaunchKernelGGL(rd_float_parse_kernel, dim3((unsigned)(wgs < FP_MAX_WGS ? wgs : FP_MAX_WGS)), dim3(FP_THREADS), 0, (hipStream_t)stream, text, start, n, bits,
                       status);
    RD_HIP(hipGetLastError());
    return RD_OK;
}

// reads longer than max_len over windows (rd_windows.hpp): the plan counts and scans, the fill writes the window table that rd_classify
// takes, the fuse turns the windows' logits into the reads'
namespace {
struct WindowWs {
    int nb;
    int64_t *bsum;
    int32_t *fault;
    size_t total;
};
WindowWs window_ws(void *workspace, int64_t n) {
    WindowWs p;
    Carver c(workspace);
    p.nb = scan_blocks(n);
    p.bsum = c.take<int64_t>((size_t)p.nb);
    p.fault = c.take<int32_t>(1);
    p.total = c.off;
    return p;
}
// the rule's parameters, as every rd_window_* entry point that takes them checks them
int window_rule_check(const char *fn, int64_t n, int32_t max_len, int64_t stride, int32_t max_windows) {
    if (n < 0 || n > 0x7fffffffLL) RD_FAIL(RD_E_INVALID, "%s: n=%lld out of range", fn, (long long)n);
    if (max_len < 1 || max_len > MAX_LEN_LIMIT) RD_FAIL(RD_E_INVALID, "%s: max_len=%d out of range [1,%d]", fn, max_len, MAX_LEN_LIMIT);
    if (stride < 1 || stride > 0x7fffffffLL) RD_FAIL(RD_E_INVALID, "%s: stride=%lld out of range [1,2^31-1]", fn, (long long)stride);
    if (max_windows < 1 || max_windows > RD_WINDOW_MAX) RD_FAIL(RD_E_INVALID, "%s: max_windows=%d out of range [1,%d]", fn, max_windows, RD_WINDOW_MAX);
    return RD_OK;
}
}  // namespace

size_t rd_window_workspace_bytes(int64_t n) {
    if (n < 0 || n > 0x7fffffffLL) return 0;
    return window_ws(nullptr, n).total;
}

int rd_window_plan(const int32_t *seq_len, int64_t n, int32_t max_len, int64_t stride, int32_t max_windows, int64_t *win_first, int64_t *info,
                   void *workspace, size_t workspace_bytes, void *stream) {
    if (const int rc = window_rule_check("rd_window_plan", n, max_len, stride, max_windows)) return rc;
    if (!info || !win_first) RD_FAIL(RD_E_INVALID, "rd_window_plan: null info or win_first");
    hipStream_t st = (hipStream_t)stream;
    if (n == 0) {
        RD_HIP(hipMemsetAsync(info, 0, 4 * sizeof(int64_t), st));
        RD_HIP(hipMemsetAsync(win_first, 0, sizeof(int64_t), st));
        return RD_OK;
    }
    if (!seq_len || !workspace) RD_FAIL(RD_E_INVALID, "rd_window_plan: null pointer");
    if ((uintptr_t)workspace & 255) RD_FAIL(RD_E_INVALID, "rd_window_plan: workspace must be 256-byte aligned");
    const WindowWs p = window_ws(workspace, n);
    if (workspace_bytes < p.total) RD_FAIL(RD_E_WORKSPACE, "rd_window_plan: workspace too small: %zu < %zu", workspace_bytes, p.total);
    RD_HIP(hipMemsetAsync(p.fault, 0, sizeof(int32_t), st));
    hipLaunchKernelGGL(rd_window_count_kernel, dim3(p.nb), dim3(256), 0, st, seq_len, n, (int64_t)max_len, stride, (int64_t)max_windows, p.bsum, p.fault);
    scan_base(p.bsum, p.nb, info, INT64_MAX, st);
    hipLaunchKernelGGL((rd_scan_off_kernel<8, 1, WnLen, WnVerdict>), dim3(p.nb), dim3(256), 0, st, WnLen{seq_len, (int64_t)max_len, stride, (int64_t)max_windows}, n,
                       ScanOut<1>{{win_first}, {p.bsum}}, WnVerdict{n, p.fault, info});
    RD_HIP(hipGetLastError());
    return RD_OK;
}

int rd_window_fill(const int64_t *seq_off, const int32_t *seq_len, const int64_t *win_first, int64_t n, int32_t max_len, int64_t stride,
                   int32_t max_windows, int64_t total, int64_t *win_off, int32_t *win_len, void *stream) {
    if (const int rc = window_rule_check("rd_window_fill", n, max_len, stride, max_windows)) return rc;
    if (total < n || total > n * (int64_t)max_windows) RD_FAIL(RD_E_INVALID, "rd_window_fill: total=%lld is not a window count of %lld reads", (long long)total, (long long)n);
    if (n == 0) return RD_OK;
    if (!seq_off || !seq_len || !win_first || !win_off || !win_len) RD_FAIL(RD_E_INVALID, "rd_window_fill: null pointer");
    hipLaunchKernelGGL(rd_window_fill_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, seq_off, seq_len, win_first, n,
                       (int64_t)max_len, stride, (int64_t)max_windows, total, win_off, win_len);
    RD_HIP(hipGetLastError());
    return RD_OK;
}

int rd_window_fuse(const float *win_logits, const int64_t *win_first, int64_t n, int32_t mode, int32_t only_multi, float *logits, uint8_t *labels,
                   void *stream) {
    if (n < 0 || n > 0x7fffffffLL) RD_FAIL(RD_E_INVALID, "rd_window_fuse: n=%lld out of range", (long long)n);
    if (mode != RD_WINDOW_MEAN && mode != RD_WINDOW_MAX_D) RD_FAIL(RD_E_INVALID, "rd_window_fuse: unknown mode %d", mode);
    if (n == 0) return RD_OK;
    if (!win_logits || !win_first || !logits) RD_FAIL(RD_E_INVALID, "rd_window_fuse: null pointer");
    if (((uintptr_t)win_logits | (uintptr_t)logits) & 7) RD_FAIL(RD_E_INVALID, "rd_window_fuse: win_logits and logits must be 8-byte aligned");
    hipLaunchKernelGGL(rd_window_fuse_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (const float2 *)win_logits, win_first, n,
                       (int)mode, (int)(only_multi != 0), (float2 *)logits, labels);
    RD_HIP(hipGetLastError());
    return RD_OK;
}

// the rRNA regions of a chunk's reads (rd_regions.hpp): per-unit tables sized by n (always for two mates), then the line table, which
// takes what is left of the workspace - rd_region_workspace_bytes leaves room for (total_windows + 2 n) / 2 lines, the most there can be
namespace {
struct RegionWs {
    int nb;
    int64_t *unit_bytes, *unit_lines, *bsum_bytes, *bsum_lines, *tot_bytes, *tot_lines;
    int32_t *idlen, *fault;
    unsigned long long *cnt;
    size_t fixed;
    int64_t line_cap;
    int64_t *line_off;
    int32_t *line_unit, *line_start, *line_end;
    uint32_t *line_wq;
};
constexpr size_t RG_LINE_SLACK = 8 + 5 * 256;     // entry `lines` of line_off, and the alignment of the five arrays
RegionWs region_ws(void *workspace, int64_t n, int64_t units, size_t workspace_bytes) {
    RegionWs p;
    Carver c(workspace);
    p.nb = scan_blocks(units, 1);
    const size_t cap_units = (size_t)(2 * n + 1), cap_nb = (size_t)scan_blocks(2 * n, 1);
    p.unit_bytes = c.take<int64_t>(cap_units);
    p.unit_lines = c.take<int64_t>(cap_units);
    p.idlen = c.take<int32_t>(cap_units);
    p.bsum_bytes = c.take<int64_t>(cap_nb);
    p.bsum_lines = c.take<int64_t>(cap_nb);
    p.tot_bytes = c.take<int64_t>(4);
    p.tot_lines = c.take<int64_t>(4);
    p.cnt = c.take<unsigned long long>(4);
    p.fault = c.take<int32_t>(1);
    p.fixed = c.off;
    p.line_cap = workspace_bytes > p.fixed + RG_LINE_SLACK ? (int64_t)((workspace_bytes - p.fixed - RG_LINE_SLACK) / 24) : 0;
    p.line_off = c.take<int64_t>((size_t)p.line_cap + 1);
    p.line_unit = c.take<int32_t>((size_t)p.line_cap);
    p.line_start = c.take<int32_t>((size_t)p.line_cap);
    p.line_end = c.take<int32_t>((size_t)p.line_cap);
    p.line_wq = c.take<uint32_t>((size_t)p.line_cap);
    return p;
}
}  // namespace

size_t rd_region_workspace_bytes(int64_t n, int64_t total_windows) {
    if (n < 0 || n > 0x3fffffffLL || total_windows < 0) return 0;
    return region_ws(nullptr, n, 2 * n, 0).fixed + RG_LINE_SLACK + 24 * (size_t)((total_windows + 2 * n) / 2 + 1);
}

int rd_region_format(const uint8_t *text_a, int64_t bytes_a, const int64_t *rec_start_a, const int32_t *seq_len_a, const int64_t *win_first_a,
                     const float *win_logits_a, const uint8_t *text_b, int64_t bytes_b, const int64_t *rec_start_b, const int32_t *seq_len_b,
                     const int64_t *win_first_b, const float *win_logits_b, int64_t rec_stride, int64_t n, int32_t max_len, uint8_t *out, size_t out_cap,
                     int64_t *info, void *workspace, size_t workspace_bytes, void *stream) {
    if (n < 0 || n > 0x3fffffffLL || bytes_a < 0 || bytes_b < 0) RD_FAIL(RD_E_INVALID, "rd_region_format: bad n or text bytes");
    if (rec_stride != 1 && rec_stride != 2) RD_FAIL(RD_E_INVALID, "rd_region_format: rec_stride must be 1 or 2; got %lld", (long long)rec_stride);
    if (max_len < 1 || max_len > MAX_LEN_LIMIT) RD_FAIL(RD_E_INVALID, "rd_region_format: max_len=%d out of range [1,%d]", max_len, MAX_LEN_LIMIT);
    if (!info) RD_FAIL(RD_E_INVALID, "rd_region_format: null info");
    hipStream_t st = (hipStream_t)stream;
    if (n == 0) {
        RD_HIP(hipMemsetAsync(info, 0, 8 * sizeof(int64_t), st));
        return RD_OK;
    }
    const int mates = text_b ? 2 : 1;
    if (!text_a || !rec_start_a || !seq_len_a || !win_first_a || !win_logits_a || !out || !workspace) RD_FAIL(RD_E_INVALID, "rd_region_format: null pointer");
    if (mates == 2 && (!rec_start_b || !seq_len_b || !win_first_b || !win_logits_b)) RD_FAIL(RD_E_INVALID, "rd_region_format: null pointer (mate 2)");
    if (((uintptr_t)workspace & 255) || ((uintptr_t)out & 15)) RD_FAIL(RD_E_INVALID, "rd_region_format: workspace must be 256-byte aligned, out 16-byte aligned");
    if (((uintptr_t)win_logits_a | (uintptr_t)win_logits_b) & 7) RD_FAIL(RD_E_INVALID, "rd_region_format: win_logits must be 8-byte aligned");
    const int64_t units = n * mates;
    const RegionWs p = region_ws(workspace, n, units, workspace_bytes);
    if (workspace_bytes < p.fixed + RG_LINE_SLACK) RD_FAIL(RD_E_WORKSPACE, "rd_region_format: workspace too small: %zu < %zu", workspace_bytes, p.fixed + RG_LINE_SLACK);
    const RgMate ma = {text_a, bytes_a, rec_start_a, seq_len_a, win_first_a, (const float2 *)win_logits_a};
    const RgMate mb = {text_b, bytes_b, rec_start_b, seq_len_b, win_first_b, (const float2 *)win_logits_b};
    const int64_t cap = (int64_t)(out_cap < (size_t)INT64_MAX ? out_cap : (size_t)INT64_MAX);
    RD_HIP(hipMemsetAsync(p.cnt, 0, (size_t)((char *)p.fault - (char *)p.cnt) + sizeof(int32_t), st));     // (the counters and the fault word)
    hipLaunchKernelGGL(rd_region_count_kernel, dim3(p.nb), dim3(256), 0, st, ma, mb, mates, rec_stride, n, (int64_t)max_len, p.unit_bytes, p.unit_lines, p.idlen,
                       p.bsum_bytes, p.bsum_lines, p.cnt, p.fault);
    scan_base(p.bsum_bytes, p.nb, p.tot_bytes, INT64_MAX, st);
    scan_base(p.bsum_lines, p.nb, p.tot_lines, INT64_MAX, st);
    hipLaunchKernelGGL((rd_scan_off_kernel<1, 2, ScanTab<2>, RgVerdict>), dim3(p.nb), dim3(256), 0, st, ScanTab<2>{{p.unit_bytes, p.unit_lines}}, units,
                       ScanOut<2>{{p.unit_bytes, p.unit_lines}, {p.bsum_bytes, p.bsum_lines}}, RgVerdict{units, p.tot_bytes, p.tot_lines, p.cnt, p.fault, cap, p.line_cap, info});
    hipLaunchKernelGGL(rd_region_lines_kernel, dim3(p.nb), dim3(256), 0, st, ma, mb, mates, n, (int64_t)max_len, p.unit_bytes, p.unit_lines, p.idlen, info, p.line_cap,
                       p.line_off, p.line_unit, p.line_start, p.line_end, p.line_wq);
    const int64_t tiles = (p.line_cap + RG_LINES - 1) / RG_LINES;
    hipLaunchKernelGGL(rd_region_write_kernel, dim3((unsigned)(tiles < 1 ? 1 : tiles > 4096 ? 4096 : tiles)), dim3(256), 0, st, ma, mb, mates, rec_stride,
                       p.unit_lines, units, p.idlen, p.line_off, p.line_unit, p.line_start, p.line_end, p.line_wq, out, info);
    RD_HIP(hipGetLastError());
    return RD_OK;
}

#ifdef RD_DIAG
// diagnostic build only (not in include/ribodetector_amd.h): [dev] uint64[32] that receives the cycles per stage of rd_gz_deflate_kernel ([0..15]) and rd_gz_inflate_kernel ([16..31])
RD_API int rd_gz_diag_set_profile(unsigned long long *dev_buf) {
    RD_HIP(hipMemcpyToSymbol(HIP_SYMBOL(g_gz_prof), &dev_buf, sizeof(dev_buf)));
    return RD_OK;
}
#endif

}  // extern "C"
