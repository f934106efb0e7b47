/*
 * ribodetector_amd.h - C ABI of the MI355X-native RiboDetector inference path (librd_hip.so).
 *
 * The reference (hzi-bifo/RiboDetector v0.3.1) is pure Python and has no FFI of its own; the seam it offers
 * is a Python duck type resolved from config.json. Each entry point below names the reference
 * interface it replaces (paths relative to /root/reference/ribodetector). INTEGRATION.md shows the ctypes
 * binding a maintainer of the reference would add.
 *
 * Conventions
 *   - plain pointers and sizes only; every pointer marked [dev] is device (HBM) memory owned by the caller,
 *     [host] is host memory. Nothing is allocated behind the caller's back except inside rd_model_create.
 *   - every launch takes an explicit hipStream_t (passed as void*; 0 = the null stream) and is asynchronous;
 *     the caller synchronises.
 *   - return value: 0 = ok, <0 = error (RD_E_*); rd_last_error() returns a thread-local message.
 *     No C++ exception crosses this boundary.
 *   - reads are handed over as raw ASCII: one byte arena + per-read start offset + per-read length
 *     (exactly what a FASTQ/FASTA chunk in memory looks like). Only the first `max_len` bases of a read are
 *     used (reference detect.py:682,714,717 `read[1][:max_len]`).
 */
#ifndef RIBODETECTOR_AMD_H
#define RIBODETECTOR_AMD_H

#include <stddef.h>
#include <stdint.h>

/* every entry point is exported explicitly: the libraries are built with -fvisibility=hidden, so `nm -D` lists exactly these */
#ifndef RD_API
#define RD_API __attribute__((visibility("default")))
#endif

#ifdef __cplusplus
extern "C" {
#endif

#define RD_OK 0
#define RD_E_INVALID (-1)   /* bad argument                                   */
#define RD_E_HIP (-2)       /* a HIP runtime call failed                      */
#define RD_E_UNSUPPORTED (-3) /* architecture / arg combination not covered   */
#define RD_E_WORKSPACE (-4) /* workspace too small                            */

/* --ensure modes of reference detect.py:616-663 */
#define RD_ENSURE_NONE 0
#define RD_ENSURE_RRNA 1
#define RD_ENSURE_NORRNA 2
#define RD_ENSURE_BOTH 3

/* LSTM kernel variants (rd_set_variant): all compute the same function within the 1e-4 logit bound */
#define RD_VARIANT_AUTO 0       /* = MFMA_F16X3_T32                                                            */
#define RD_VARIANT_MFMA_F32 1   /* persistent-weight fp32 MFMA recurrence (v_mfma_f32_16x16x4_f32)              */
#define RD_VARIANT_SIMPLE 2     /* plain fp32 FMA kernel, correctness cross-check                              */
/* id 3 (the first 16x16x32 tiling of the split-precision kernel) was removed in 0.2: RD_E_UNSUPPORTED          */
#define RD_VARIANT_MFMA_F16X3_T32 4 /* fp32 product as 3 fp16 MFMA products (hi*hi + hi*lo + lo*hi) on v_mfma_f32_32x32x16_f16,
                                       fp32 accumulate, 32-read tiles, hand-interleaved gate math                */
/* Any other id is rejected with RD_E_UNSUPPORTED by librd_hip.so. The A/B and diagnostic instantiations used by tools/
 * (ids >= 10, some of them wrong by design) exist only in the separately built librd_hip_diag.so (-DRD_DIAG). */

/* output-row semantics (rd_set_semantics) */
#define RD_SEM_PACKED 0 /* reference GPU product: PackedSequence, gather at timestep min(len,max_len)-1 (model/model.py:32-37)  */
#define RD_SEM_PADDED 1 /* reference CPU product `ribodetector_cpu`: input zero-padded to max_len rows, BiLSTM over all rows,
                           gather at the last non-zero row (model/model_cpu.py:29-37,57-62, detect_cpu.py:699-700)            */

typedef struct rd_model rd_model; /* opaque: device-resident, pre-packed weights */

/* Host pointers to the 10 tensors of the reference state_dict (reference model/model.py:16-24; names as in
 * torch: rnn.weight_ih_l0 [4H,I], rnn.weight_hh_l0 [4H,H], rnn.bias_ih_l0 [4H], rnn.bias_hh_l0 [4H], the same
 * four with suffix _reverse, out.weight [C,2H], out.bias [C]); row-major fp32, torch gate order i,f,g,o. */
typedef struct rd_weights {
    const float *w_ih, *w_hh, *b_ih, *b_hh;
    const float *w_ih_r, *w_hh_r, *b_ih_r, *b_hh_r;
    const float *w_out, *b_out;
    int32_t input_size;   /* must be 4   */
    int32_t hidden_size;  /* must be 128 */
    int32_t num_classes;  /* must be 2   */
} rd_weights;

/* Replaces: SeqModel(**arch.args); load_state_dict(...); .to('cuda'); .eval()
 * (reference detect.py:93,115-119, model/model.py:10-29). Uploads the weights to `device` and pre-packs them
 * (per-lane MFMA operand order for W_hh, fused input table  W_ih[:,base]+b_ih+b_hh, reverse-direction table).
 * Synchronous.
 * Accepted weights (checked on the host before any device call; rd_weights_check is that check alone and needs no GPU):
 *   - every value of every tensor is finite, else RD_E_INVALID (the message names the tensor);
 *   - max |rnn.weight_hh_l0| < 65504 / 16 = 4094, else RD_E_UNSUPPORTED: the split-precision kernel stores 16 w in fp16, whose
 *     largest finite value is 65504 (a larger weight would become inf there and every logit NaN).
 *   Gates and cell states that saturate the activations are inside the range: tests/test_gpu_weights.py holds every kernel to
 *   the reference's own fp32 error on weights with pre-activations beyond +-100 and |c| up to 300. */
RD_API int rd_weights_check(const rd_weights *w);
RD_API int rd_model_create(const rd_weights *w, int device, rd_model **out);
RD_API void rd_model_destroy(rd_model *m);

/* Select the recurrence kernel (RD_VARIANT_*); default AUTO = MFMA_F16X3_T32. Ids this build does not contain are
 * refused with RD_E_UNSUPPORTED (the model keeps its current kernel). rd_variant_available: 1 if `variant` can be selected. */
RD_API int rd_set_variant(rd_model *m, int variant);
RD_API int rd_variant_available(int variant);

/* Select which of the reference's two products rd_classify reproduces (RD_SEM_*); default RD_SEM_PACKED. The two differ
 * only for reads shorter than max_len or ending in non-ACGT bases. */
RD_API int rd_set_semantics(rd_model *m, int semantics);

/* Label stability. The label is argmax(logits) (reference detect.py:288,481); every fp32 evaluation of the recurrence - the
 * reference's own included - carries up to ~1e-4 of rounding noise on the logits, so for the few reads per million whose margin
 * |logit1 - logit0| is smaller than that the label is decided by noise. rd_classify therefore re-evaluates every read whose
 * margin is below `thresh` (default RD_REFINE_DEFAULT, ~15 reads per million) in float64 - the same function, reference
 * model/model.py:32-37, with all products, sums and activations in double - and replaces its logits and label: labels are
 * those of the exact function, independent of kernel variant and batch split. thresh = 0 switches the pass off.
 * rd_refine is the same pass as a separate call (thresh <= 0: the model's band):
 *   - for callers that hold logits of BOTH mates: with `mate_logits` ([dev] float[n*2], row i = the mate of read i) a read is
 *     also re-evaluated when the PAIR margin |(l1+m1) - (l0+m0)| is below 2*thresh, which is what decides the pair label under
 *     --ensure none (detect.py:657); call it once per mate before rd_pair_fuse;
 *   - for throughput: the pass has the latency of one read (~0.3 ms: 100 dependent float64 steps on one CU) with the rest of
 *     the GPU idle. A pipelined caller switches the inline pass off (rd_set_refine(m, 0)) and issues rd_refine(..., thresh)
 *     on a second stream, where it overlaps the next batch's recurrence (bench.py and the CLI do).
 * One launch: each workgroup scans 512 logit rows and re-evaluates the candidates among them itself.
 * rd_set_refine_async(m, K), K in [1, 16], moves the pass off the caller's critical path without a second stream on the caller's
 * side (opt-in; 0 = back to the inline pass): rd_classify then only RECORDS its candidates (where their bases lie, where their
 * results go) in a queue the model owns, and the candidates of K consecutive calls are evaluated together - one workgroup each, so
 * all of them in the 0.3 ms one takes - on a stream the model owns, beside the recurrence of the call that follows the group.
 * A call's logits / labels are final, and its input buffers may be overwritten, for work issued on the caller's stream
 *   (a) after the K-th call that follows it has been issued (K = 1: after the next call), or
 *   (b) after rd_sync_results(m, stream) - which evaluates whatever waits, on the model's stream, and makes `stream` wait for it.
 *       `stream` need not be the stream the calls were issued on, as long as it is ordered behind them (an event): a pipelined
 *       caller gives its post-processing stream, so that the evaluation and what consumes it (pair fusion, label D2H) run beside the
 *       next batch's recurrences while the calls' own stream never waits (bench.py and the CLI do, since round 4). Calls issued
 *       after it record into the model's other queue. All rd_classify calls of a model in this mode go to ONE stream.
 * Until then the buffers of those calls must stay as they are: a streaming caller cycles K + 1 sets of buffers and consumes the
 * results of a call K calls later (what the reference's loop cannot do: it synchronises on .tolist() every batch, reference
 * detect.py:288,481). A call that passes a pointer of a waiting call, or overlapping output ranges, is detected and synchronises
 * first (correct results, no overlap). rd_refine synchronises first too. A call captured in a hipGraph keeps the pass inline.
 * Candidates beyond the queue's 8,192 entries are evaluated inside rd_classify. rd_model_destroy / changing K require
 * rd_sync_results first (candidates still waiting at destroy keep their fp32 results). */
#define RD_REFINE_DEFAULT 2.5e-4f
RD_API int rd_set_refine(rd_model *m, float thresh);
RD_API int rd_set_refine_async(rd_model *m, int calls_per_group);
RD_API int rd_sync_results(rd_model *m, void *stream);
RD_API int rd_refine(const rd_model *m, const uint8_t *arena, const int64_t *seq_off, const int32_t *seq_len, int64_t n,
              int32_t max_len, float *logits, uint8_t *labels, const float *mate_logits, float thresh, void *stream);

/* Prefix-state table (an extension; nothing in the reference to replace - its cuDNN call steps over every
 * base, reference model/model.py:33). The forward recurrence is a pure function of the bases read so far, and there are only 4^k
 * sequences of k bases: row p of the table is the recurrence state (h as the kernel's two fp16 arrays, the cell state in fp32;
 * 1 KiB) after the k bases whose base-4 number is p, computed by the classifying kernel itself, so that a read whose first k bases
 * are A/C/G/T(U) starts from its row and runs min(len,max_len) - k steps with bit-identical results (reads with another letter in
 * the prefix, or no step left after it, run all their steps from the zero state as before). This is the reverse-direction table
 * (one step, 5 rows) carried k steps forward: k = 12 takes 16 GiB of the 288 GB of HBM and removes 12 % of the steps of a 100 bp read.
 *   rd_prefix_table_bytes(k): bytes of [dev] memory for k in [RD_PREFIX_K_MIN, RD_PREFIX_K_MAX] ((4^k + 1) KiB); 0 otherwise.
 *   rd_prefix_scratch_bytes(k): bytes of [dev] scratch the build needs (4^(k-1) KiB: the level below), free again afterwards.
 *   rd_set_prefix_table: builds the table for the model's weights into caller-owned `table` (256-byte aligned, >= that many
 *     bytes; it must stay allocated until the model is destroyed or another / no table is set) and attaches it: k launches, level
 *     j = the states after every j-base prefix from level j-1 by ONE step (4/3 4^k steps in all: 15 ms at k = 12). k = 0 (pointers
 *     may be NULL) detaches. Synchronous on `stream`. The rows are the state of the kernel that builds them - the model's CURRENT
 *     variant: RD_VARIANT_MFMA_F16X3_T32 (h as two fp16 arrays + fp32 cell state) or RD_VARIANT_MFMA_F32 (h and c in fp32; same 1 KiB,
 *     same addressing); RD_VARIANT_SIMPLE has none (RD_E_UNSUPPORTED). rd_classify uses the table only while the model's variant is
 *     the one that built it (after rd_set_variant to another kernel the reads run all their steps until the table is rebuilt).
 *   rd_prefix_k: k of the attached table, 0 if none. */
#define RD_PREFIX_K_MIN 4
#define RD_PREFIX_K_MAX 13
RD_API size_t rd_prefix_table_bytes(int32_t k);
RD_API size_t rd_prefix_scratch_bytes(int32_t k);
RD_API int rd_set_prefix_table(rd_model *m, int32_t k, void *table, size_t table_bytes, void *scratch, size_t scratch_bytes, void *stream);
RD_API int rd_prefix_k(const rd_model *m);

/* Bytes of [dev] scratch rd_classify needs for n reads with truncation length max_len. */
RD_API size_t rd_classify_workspace_bytes(int64_t n, int32_t max_len);

/* Replaces: collate (one-hot + pack_sequence, reference detect.py:666-689) + model(x) (model/model.py:32-37
 * forward1: BiLSTM over min(len,max_len) steps, last-timestep gather, Linear) + torch.argmax (detect.py:288,481).
 *   arena   [dev] ASCII bytes;  seq_off [dev] int64[n] start of read i in arena;  seq_len [dev] int32[n]
 *   logits  [dev] float[n*2], row i <-> read i (input order);  labels [dev] uint8[n] or NULL (1 = rRNA)
 *   workspace [dev] >= rd_classify_workspace_bytes(n, max_len), 256-byte aligned */
RD_API int rd_classify(const rd_model *m, const uint8_t *arena, const int64_t *seq_off, const int32_t *seq_len, int64_t n,
                int32_t max_len, float *logits, uint8_t *labels, void *workspace, size_t workspace_bytes, void *stream);

/* Replaces: Predictor.separate_paired_reads label logic (reference detect.py:616-663).
 *   logits1/logits2 [dev] float[n*2];  pair_labels [dev] int8[n] in {0,1,-1}
 *   counts [dev] uint64[3] or NULL: (non-rRNA, rRNA, unclassified) ADDED to the existing values
 *   (the running counters of detect.py:331-333,388-389,400). */
RD_API int rd_pair_fuse(const float *logits1, const float *logits2, int64_t n, int32_t ensure_mode, int8_t *pair_labels,
                 uint64_t *counts, void *stream);

/* Replaces: Predictor.separate_reads counters for single-end (reference detect.py:600-614,485-486).
 *   labels [dev] uint8[n]; counts [dev] uint64[3], ADDED to. */
RD_API int rd_count_labels(const uint8_t *labels, int64_t n, uint64_t *counts, void *stream);

/* Replaces: SeqEncoder.encode_read / BASE_DICT (reference data_loader/seq_encoder.py:11-18,126-127) for a batch.
 * codes [dev] uint8[n*stride]: 0 A, 1 C, 2 G, 3 T/U, 4 anything else; positions >= min(len,max_len) hold 4.
 * stride >= max_len. */
RD_API int rd_encode_codes(const uint8_t *arena, const int64_t *seq_off, const int32_t *seq_len, int64_t n, int32_t max_len,
                    int32_t stride, uint8_t *codes, void *stream);

/* Replaces: encode_variable_len_read + np.array(..., float32) (reference seq_encoder.py:130-145,
 * detect_cpu.py:699-700): onehot [dev] float[n*max_len*4], zero rows after the read. */
RD_API int rd_encode_onehot_padded(const uint8_t *arena, const int64_t *seq_off, const int32_t *seq_len, int64_t n,
                            int32_t max_len, float *onehot, void *stream);

/* Replaces: torch.FloatTensor(encode_read(...)) + pack_sequence(enforce_sorted=False) (reference
 * detect.py:681-685). Two calls:
 *   rd_pack_plan: fills sorted_idx [dev] int64[n] (lengths descending, ties by input index), unsorted_idx [dev]
 *     int64[n], batch_sizes [dev] int64[max_len] (entries past the longest read are 0) and total_steps [dev]
 *     int64[1] = sum_i min(len_i,max_len).  workspace as for rd_classify. API parity only: rd_classify does NOT call it (it
 *     buckets by step count with atomics, order inside a bucket free).
 *   rd_pack_onehot: writes data [dev] float[total_steps*4], time-major over the sorted reads. */
RD_API int rd_pack_plan(const int32_t *seq_len, int64_t n, int32_t max_len, int64_t *sorted_idx, int64_t *unsorted_idx,
                 int64_t *batch_sizes, int64_t *total_steps, void *workspace, size_t workspace_bytes, void *stream);
RD_API int rd_pack_onehot(const uint8_t *arena, const int64_t *seq_off, const int32_t *seq_len, int64_t n, int32_t max_len,
                   const int64_t *sorted_idx, const int64_t *batch_sizes, float *data, void *stream);

/* Device-side gzip of the output files (round 4). Replaces, for the GPU path: gzip.open(out, 'wt', compresslevel=5) fed with the
 * records of one label in input order (reference detect.py:485-492,729-741: the writer compresses by file extension). The records of
 * a chunk (its text is already in HBM: the read bytes travel as the chunk's text) whose label equals `label` become a sequence of
 * complete gzip members in `out`, ready to be appended to the file - in BGZF framing (one member per 65,280 input bytes, 'B','C'
 * extra subfield), so that the file is also what bgzip writes: indexable, and decodable member by member in parallel. DEFLATE is
 * done by hand-written kernels: LZ77 with per-wave hash tables in LDS, one dynamic-Huffman block per member, CRC-32 on the device.
 *   text [dev] the chunk's bytes; rec_start [dev] int64[n+1]: record i = bytes [rec_start[i], rec_start[i+1]) (verbatim, with its
 *   newline); labels [dev] int8[n] (rd_pair_fuse's pair labels, or rd_classify's uint8 labels); label: the value to select.
 *   out [dev] >= rd_gz_out_bound(text_bytes) bytes is always enough (256-byte aligned); info [dev] int64[4]:
 *     info[0] = bytes written to out (if > out_cap: out was too small and is incomplete), info[1] = uncompressed bytes,
 *     info[2] = members, info[3] != 0: rec_start does not describe `text` (the selected records hold more bytes than the text:
 *     nothing was compressed). Asynchronous on `stream`; the caller copies info and out[0, info[0]) to the host afterwards.
 *   rd_gz_eof_block: [host] BGZF's 28-byte end-of-file marker (an empty member), to be appended once when the file is closed. */
RD_API size_t rd_gz_workspace_bytes(int64_t n, int64_t text_bytes);
RD_API size_t rd_gz_out_bound(int64_t text_bytes);
RD_API int rd_gz_compress_selected(const uint8_t *text, int64_t text_bytes, const int64_t *rec_start, const int8_t *labels, int64_t n,
                            int32_t label, uint8_t *out, size_t out_cap, int64_t *info, void *workspace, size_t workspace_bytes,
                            void *stream);
RD_API int rd_gz_eof_block(uint8_t *dst, size_t cap);

/* The input side of the same idea (round 4): a .gz whose members say how long they are - BGZF (bgzip / htslib, and every .gz this
 * build's CLI writes) - is a list of independent DEFLATE streams, and they are inflated on the device, one wave per member
 * (replaces, for such files: gzip.open(path, 'rt') in reference data_loader/seq_encoder.py:21-39 / fastx_parser.py:15-55). The host
 * walks the member headers (no decoding needed: the size is in the 'B','C' subfield, ISIZE in the trailer) and fills one rd_gz_member
 * per member; every DEFLATE block type is handled; each member's CRC-32 and ISIZE are checked on the device.
 *   comp [dev] the compressed bytes (at least 8 readable bytes behind the last member's data: its trailer);
 *   members [dev] rd_gz_member[n] (in_len at most 256 MiB; an entry that points outside comp / text gets RD_GZI_MEMBER, nothing is read
 *   or written for it); text [dev] receives member i's out_len bytes at out_off;
 *   status [dev] uint32[n]: 0 = ok, else RD_GZI_* (the member's output is then undefined). Asynchronous on `stream`. */
typedef struct rd_gz_member {
    int64_t in_off;   /* first byte of the member's raw DEFLATE data in comp (behind the gzip header) */
    int64_t out_off;  /* where its bytes go in text */
    int32_t in_len;   /* bytes of raw DEFLATE data; the 8-byte trailer (CRC-32, ISIZE) follows them */
    int32_t out_len;  /* ISIZE */
} rd_gz_member;
#define RD_GZI_OK 0
#define RD_GZI_BAD_BLOCK 1
#define RD_GZI_BAD_CODE 2
#define RD_GZI_BAD_LENGTHS 3
#define RD_GZI_OVERRUN 4
#define RD_GZI_BAD_DISTANCE 5
#define RD_GZI_TRUNCATED 6
#define RD_GZI_SIZE 7
#define RD_GZI_CRC 8
#define RD_GZI_STORED 9
#define RD_GZI_MEMBER 10   /* the descriptor itself: offsets / lengths outside comp or text */
RD_API int rd_gz_inflate_members(const uint8_t *comp, int64_t comp_bytes, const rd_gz_member *members, int64_t n, uint8_t *text, int64_t text_bytes,
                          uint32_t *status, void *stream);

/* The FASTQ record index, on the device (round 5). Replaces, for text that already lies in HBM - BGZF members inflated there by
 * rd_gz_inflate_members, or a plain file's bytes copied there - the parser's FASTQ state machine (reference
 * data_loader/fastx_parser.py:15-37: four lines per record, each rstrip()-ed, header / '+' / quality verbatim, bases not upper-cased),
 * so that inflate -> index -> classify -> select -> deflate never returns text to the host. The stream arrives in batches; a batch
 * buffer `text` [dev] has `pad` spare bytes in front of its new bytes [pad, end) and >= 65 readable / writable bytes behind `end`:
 *   rd_fastq_index: the bytes behind the last complete record of the batch before (prev_text / prev: that batch's buffer and its
 *     summary, both [dev], read on the device - or both NULL for the first batch) are copied in front of `pad`; the window [begin,
 *     end) is framed: line_end [dev] int32[cap_lines] receives the offset in `text` of the '\n' ending line j (cap_lines >= end - pad
 *     + carry + 1 is always enough); record r = lines 4r .. 4r + 3, its text = [start of line 4r, line_end[4r + 3] + 1), its bases =
 *     line 4r + 1. final != 0: the stream ends with this batch - a last line without '\n' gets one, and fewer than four trailing lines
 *     are tolerated when blank. summary [dev] rd_fq_summary: status RD_FQ_* (HEADER: record `bad_record` does not start with '@';
 *     TRUNCATED: the stream ends inside a record; CARRY: a record longer than `pad`; CHAIN: the batch before had failed);
 *     dirty != 0: some line has trailing whitespace (CR LF files) - the records are NOT verbatim ranges then: the caller strips the
 *     window (rd_fastq_strip_mark + a compaction of the marked bytes) and indexes the result with final = 1; `consumed` / `end`
 *     of the ORIGINAL summary stay the carry of the next batch. Asynchronous on `stream`; no host round trip between batches.
 *   rd_fastq_gather: records [rec_lo, rec_hi) of an indexed batch appended to a chunk: their text is copied to out_text [dev,
 *     16-byte aligned] at *cursor_in [dev] and *cursor_out [dev, another address] = the position behind it (-1 if it did not fit
 *     out_cap, or the batch / the cursor was bad: every later piece then fails too); rec_start [dev] int64[rec_hi - rec_lo + 1],
 *     seq_off int64[..], seq_len int32[..] = the chunk's entries for these records (offsets into out_text) - the arrays rd_classify and
 *     rd_gz_compress_selected take. max_bytes: an upper bound of the bytes (sizes the launch), e.g. the batch's window size.
 *   rd_fastq_strip_mark: del [dev, zeroed by the caller] gets 1 at every byte rstrip() removes from lines [0, n_lines) of the batch.
 *   rd_fastq_sample: samples [dev] int32[cap]: samples[k] = offset in `text` where record k * every starts (-1 beyond the batch's
 *     records; entry n / every ... the summary's `consumed` closes the last interval): copied to the host with the summary, they bound
 *     the bytes of any record range, so that a caller sizes a chunk's buffer without a round trip per range. */
typedef struct rd_fq_summary {
    int64_t begin, end;       /* the window framed: [begin, end) in the batch buffer (begin = pad - carry; end includes an added '\n') */
    int64_t n_lines, n_records;
    int64_t consumed;         /* offset behind the last complete record (final: = end): the next batch's carry is [consumed, end) */
    uint64_t bad_record;      /* ~0, or the first record whose header line does not start with '@' */
    int32_t status, dirty;
    int64_t reserved;
} rd_fq_summary;
#define RD_FQ_OK 0
#define RD_FQ_HEADER 1
#define RD_FQ_TRUNCATED 2
#define RD_FQ_CARRY 3
#define RD_FQ_CHAIN 4
#define RD_FQ_LINES 5      /* more lines than cap_lines */
RD_API size_t rd_fastq_index_workspace_bytes(int64_t text_end);
RD_API int rd_fastq_index(uint8_t *text, int64_t pad, int64_t end, const uint8_t *prev_text, const rd_fq_summary *prev, int32_t final, int32_t *line_end,
                   int64_t cap_lines, rd_fq_summary *summary, void *workspace, size_t workspace_bytes, void *stream);
RD_API int rd_fastq_gather(const uint8_t *text, const int32_t *line_end, const rd_fq_summary *summary, int64_t rec_lo, int64_t rec_hi, int64_t max_bytes,
                    uint8_t *out_text, int64_t out_cap, const int64_t *cursor_in, int64_t *cursor_out, int64_t *rec_start, int64_t *seq_off,
                    int32_t *seq_len, void *stream);
RD_API int rd_fastq_sample(const int32_t *line_end, const rd_fq_summary *summary, int64_t every, int32_t *samples, int64_t cap, void *stream);
RD_API int rd_fastq_strip_mark(const uint8_t *text, const int32_t *line_end, const rd_fq_summary *summary, int64_t max_lines, uint8_t *del, void *stream);

/* FASTA records on the device (round 5). Replaces the FASTA half of the parser for text that lies in HBM (reference
 * data_loader/fastx_parser.py:39-55: every line strip()-ed, blank lines skipped, '>' starts a record, the other lines of a record joined
 * and upper-cased; a record is yielded at the next header, at the end of the file only if its sequence is not empty) together with the
 * writer's '\n'.join(record) + '\n' (detect.py:489-492). A FASTA record is not a verbatim range of its file, so the batch is
 * RE-WRITTEN: norm [dev, norm_cap bytes, 16-byte aligned] receives header '\n' SEQUENCE '\n' per record (what the host reader puts into
 * its chunk buffer), rec_tab [dev] int64[cap_records] the offset in `norm` where record r starts (entry n_records = the end),
 * hdr_tab [dev] int32[cap_records] the length of its header line. text / pad / end / prev_text / prev / final / line_end / cap_lines /
 * summary as rd_fastq_index (the batches of a stream chain the same way: the carry is the raw text from the last header line on - that
 * record is complete only in a final batch; final = 2: the stream is a SHARE of a file that goes on behind it - its last record counts
 * even without a sequence, which final = 1, the end of the file, drops like the reference); summary->reserved = the bytes of `norm` that belong to records; status RD_FQ_LINES also
 * when norm_cap or cap_records is too small (norm_cap >= window + lines + 2, cap_records >= lines + 2 is always enough). Sequence lines
 * in front of the first header (a malformed file) become part of the first record's sequence, a stream without any header ONE record with
 * an empty header line - what the reference's parser yields. rd_fasta_gather / rd_fasta_sample: as rd_fastq_gather / rd_fastq_sample,
 * over `norm` and the two tables. */
RD_API size_t rd_fasta_index_workspace_bytes(int64_t text_end, int64_t cap_lines);
RD_API int rd_fasta_index(uint8_t *text, int64_t pad, int64_t end, const uint8_t *prev_text, const rd_fq_summary *prev, int32_t final, int32_t *line_end,
                   int64_t cap_lines, uint8_t *norm, int64_t norm_cap, int64_t *rec_tab, int32_t *hdr_tab, int64_t cap_records, rd_fq_summary *summary,
                   void *workspace, size_t workspace_bytes, void *stream);
RD_API int rd_fasta_gather(const uint8_t *norm, const int64_t *rec_tab, const int32_t *hdr_tab, const rd_fq_summary *summary, int64_t rec_lo, int64_t rec_hi,
                    int64_t max_bytes, uint8_t *out_text, int64_t out_cap, const int64_t *cursor_in, int64_t *cursor_out, int64_t *rec_start,
                    int64_t *seq_off, int32_t *seq_len, void *stream);
RD_API int rd_fasta_sample(const int64_t *rec_tab, const rd_fq_summary *summary, int64_t every, int32_t *samples, int64_t cap, void *stream);

/* BAM records on the device: the inflated bytes of a BAM file behind its header (BGZF members inflated by rd_gz_inflate_members, or
 * host-inflated bytes copied there) framed and RE-WRITTEN as FASTQ text - '@' name '\n' SEQ '\n' '+' '\n' QUAL '\n' per record, the rule of
 * ribodetector_amd/bam.py: 4-bit bases to letters, quality min(q, 93) + 33 ('"' where absent), flag 0x10 reverse-complemented, flag 0x900
 * (secondary / supplementary) skipped. text / pad / end / prev_text / prev / final / summary as rd_fastq_index: the carry is the raw
 * bytes behind the last complete record. norm / rec_tab / hdr_tab as rd_fasta_index, over four-line records: hdr_tab[r] = the length of
 * the header line ('@' included), the bases of record r = [rec_tab[r] + hdr_tab[r] + 1, + (record bytes - hdr_tab[r] - 5) / 2).
 * norm_cap >= 4 * (end - begin) / 3 + 64 and cap_records >= (end - begin) / 37 + 2 are always enough; smaller ones: RD_FQ_LINES.
 * summary: n_records = records delivered, n_lines = records walked (the skipped ones included), reserved = bytes of `norm`, dirty =
 * the segments of RD_BAM_SEGMENT bytes (counted from `begin`) whose speculative framing the in-order pass had to repeat (the tables
 * are those of a serial walk whatever that number is); status RD_BAM_RECORD: record `bad_record` (counting walked records) is
 * ill-formed - block_size < 32, lengths that do not fit in it, an empty name or one without its NUL; RD_BAM_TRUNCATED: a final batch
 * ends inside a record. In both the n_records in front of the damage are in the tables and can be gathered. No length of the data
 * is followed outside [begin, end). rd_bam_gather / rd_bam_sample: as rd_fasta_gather / rd_fasta_sample. */
#define RD_BAM_RECORD 6
#define RD_BAM_TRUNCATED 7
#define RD_BAM_SEGMENT 32768
RD_API size_t rd_bam_index_workspace_bytes(int64_t text_end);
RD_API int rd_bam_index(uint8_t *text, int64_t pad, int64_t end, const uint8_t *prev_text, const rd_fq_summary *prev, int32_t final, uint8_t *norm,
                 int64_t norm_cap, int64_t *rec_tab, int32_t *hdr_tab, int64_t cap_records, rd_fq_summary *summary, void *workspace,
                 size_t workspace_bytes, void *stream);
RD_API int rd_bam_gather(const uint8_t *norm, const int64_t *rec_tab, const int32_t *hdr_tab, const rd_fq_summary *summary, int64_t rec_lo, int64_t rec_hi,
                  int64_t max_bytes, uint8_t *out_text, int64_t out_cap, const int64_t *cursor_in, int64_t *cursor_out, int64_t *rec_start,
                  int64_t *seq_off, int32_t *seq_len, void *stream);
RD_API int rd_bam_sample(const int64_t *rec_tab, const rd_fq_summary *summary, int64_t every, int32_t *samples, int64_t cap, void *stream);

/* A BAM file shared by the ranks of a run (detect.py --bam_shard): where a record starts behind an arbitrary offset of the inflated
 * bytes, and how many records a share holds. The rule of both is ribodetector_amd/bam.py (find_record_start, records).
 * rd_bam_find_start: text [dev, 16-byte aligned] holds the window [0, end) of inflated bytes, end < 2^31; every offset of [lo, hi)
 * (0 <= lo <= hi <= end) is a CANDIDATE. A candidate is CONFIRMED when it and the next RD_BAM_CONFIRM - 1 records of the chain from
 * it each carry the signature of a record (block_size in 33 .. 2^26, refID / pos / next_refID / next_pos >= -1, lengths that fit in
 * block_size, a name of printable bytes that ends in NUL) and lie in front of `end` as a whole, or when the chain reaches exactly
 * `end` behind at least one such record and at_eof != 0 (the window ends where the file's data ends). It is REJECTED when a record of
 * its chain fails, and UNDECIDED when the window ends before either (at_eof == 0 only). info [dev] int64[4]: info[0] = the smallest
 * confirmed candidate or -1, info[1] = the smallest undecided one or -1, info[2] = 0, info[3] != 0: bad lo / hi / end, nothing was
 * searched. A caller accepts info[0] only when info[1] is -1 or larger, and looks again with more bytes otherwise. The answer is a
 * record start unless RD_BAM_CONFIRM records in a row are imitated by the payload of one; it need not be the first one behind lo (a
 * record of more than 64 MiB does not carry the signature). No byte at or behind `end` is read, whatever the data says.
 * rd_bam_count: the contract of rd_bam_index without norm, the tables and the text: the same walk from the same carry (text / pad /
 * end / prev_text / prev / final as there), the same summary - n_records delivered, n_lines walked, consumed, status (RD_FQ_LINES
 * cannot occur), bad_record, dirty, reserved = the bytes of FASTQ text the records would become. */
#define RD_BAM_CONFIRM 8
RD_API int rd_bam_find_start(const uint8_t *text, int64_t lo, int64_t hi, int64_t end, int32_t at_eof, int64_t *info, void *stream);
RD_API size_t rd_bam_count_workspace_bytes(int64_t text_end);
RD_API int rd_bam_count(uint8_t *text, int64_t pad, int64_t end, const uint8_t *prev_text, const rd_fq_summary *prev, int32_t final, rd_fq_summary *summary,
                 void *workspace, size_t workspace_bytes, void *stream);

/* The delivered records of a framed BAM batch as they stand in the input - block_size, fixed fields, name, CIGAR, packed bases,
 * qualities and every tag, nothing decoded - next to their FASTQ text (the rule: ribodetector_amd/bam.py select). The skipped records
 * lie between them, so the raw view is a table and a gather. rd_bam_index_src [host, no launch]: the address of the table of source
 * offsets (int32 per delivered record, offsets in `text`) that the rd_bam_index call with this workspace and this `end` filled; valid
 * as long as the caller keeps the workspace; NULL for a bad argument. rd_bam_raw_tab: raw_tab [dev] int64[cap_records] (cap_records
 * as given to rd_bam_index) = the exclusive scan of 4 + block_size over the delivered records, raw_tab[n_records] = their total;
 * samples [dev] int32[cap_samples]: samples[k] = raw_tab[min(k * every, n_records)] (closed by the total; -1 everywhere for a batch
 * that is not framed). A batch whose status is not RD_FQ_OK / RD_BAM_RECORD / RD_BAM_TRUNCATED: nothing is read or written but the
 * samples. rd_bam_raw_gather: the contract of rd_bam_gather - records [rec_lo, rec_hi) appended to out [dev, 16-byte aligned] at
 * *cursor_in; *cursor_out = the position behind them, or -1 (and nothing written) when they do not fit out_cap, the cursor was -1
 * already or the batch is not framed; raw_start[0 .. rec_hi - rec_lo] = their offsets in `out`. No byte of `out` in front of *cursor_in
 * or behind *cursor_out is written: two pieces of one chunk are two launches. max_bytes: an upper bound of the piece (sizes the grid). */
RD_API int32_t *rd_bam_index_src(void *workspace, int64_t text_end);
RD_API int rd_bam_raw_tab(const uint8_t *text, const int32_t *src_tab, const rd_fq_summary *summary, int64_t *raw_tab, int64_t cap_records, int64_t every,
                   int32_t *samples, int64_t cap_samples, void *stream);
RD_API int rd_bam_raw_gather(const uint8_t *text, const int32_t *src_tab, const int64_t *raw_tab, const rd_fq_summary *summary, int64_t rec_lo, int64_t rec_hi,
                      int64_t max_bytes, uint8_t *out, int64_t out_cap, const int64_t *cursor_in, int64_t *cursor_out, int64_t *raw_start, void *stream);

/* The records of a chunk that carry one label as ONE contiguous text in `out` [dev, 16-byte aligned], in input order - what the
 * reference's writer joins on the host (detect.py:485-492: fh.write('\n'.join(selected) + '\n')) - for plain (uncompressed) outputs of
 * chunks whose text lives on the device; arguments as rd_gz_compress_selected. info [dev] int64[4]: info[1] = bytes written,
 * info[3] != 0: the selection holds more bytes than the text or than out_cap (nothing written). */
RD_API size_t rd_select_workspace_bytes(int64_t n);
RD_API int rd_select_pack(const uint8_t *text, int64_t text_bytes, const int64_t *rec_start, const int8_t *labels, int64_t n, int32_t label, uint8_t *out,
                   size_t out_cap, int64_t *info, void *workspace, size_t workspace_bytes, void *stream);

/* The records of a chunk partitioned by KEY (outputs per read group, an extension): ONE call writes, for every key k in 0 .. K - 1, the
 * records that carry it - in input order, the same bytes rd_select_pack / rd_gz_compress_selected write for them - as one contiguous
 * run of `out`, the runs in key order. The number of launches does not depend on K. text / text_bytes / rec_start as rd_select_pack;
 * keys [dev] int32[n]: -1 = no run takes the record. 1 <= K <= RD_GROUP_KEYS_MAX.
 * rd_group_keys: the keys of a run that splits every class's file by the read group of MATE 1. rows [dev] int32 as rd_bam_group_rows
 *   writes them (0 <= G <= RD_SPLIT_GROUPS_MAX declared groups; rows G, G + 1 and G + 2 - no tag, an undeclared value, malformed tags -
 *   share member G of a family); unit u = record first + stride * u of that table, as in rd_bam_group_accumulate; labels [dev] int8[n]
 *   in {-1, 0, 1}; class_slot [host] int32[3]: the index among this mate's families of the file set of class label + 1, -1 = the
 *   class is not written. key = class_slot[label + 1] * (G + 1) + min(row, G), or -1. mate = -1: keys [dev] int32[n], a key per unit;
 *   mate = 0 / 1: keys [dev] int32[2n] over the records of an interleaved chunk, keys[2u + mate] = the key and the other mate's entry =
 *   -1 (the analogue of RD_LABEL_SKIP). info [dev] int64[4]: info[0] != 0 = a label outside -1..1 (bit 0) or a row outside 0..G + 2
 *   (bit 1): such units get -1 and the keys are not to be used; info[1] = n.
 * rd_group_pack: out [dev, 16-byte aligned]; every run STARTS on a multiple of 16 bytes. key_tab [dev] int64[K][4] = {offset of the
 *   run in out, bytes, records, 0}. info [dev] int64[4]: info[0] = records with a key, info[1] = the bytes of `out` in use (the end of
 *   the last run that holds a byte), info[3] = fault bits - 1: a key outside -1..K - 1, 2: the record table does not describe the text
 *   (an entry outside it, descending entries, or more bytes in the keyed records than text_bytes), 4: info[1] > out_cap. On any fault
 *   nothing is written or nothing in out is to be trusted; on fault 4 alone info[1] and key_tab still say what was needed.
 * rd_gz_compress_grouped: the same partition, every run a sequence of complete BGZF members of at most 65,280 input bytes; no member
 *   holds bytes of two keys. out [dev, 256-byte aligned] is compact and in key order: one copy to the host serves every file.
 *   key_tab[k] = {offset of the key's first member in out, compressed bytes, records, members}, members = ceil(text bytes of k /
 *   65,280) - 0 for a key without bytes. info[0] = compressed bytes, info[1] = uncompressed bytes, info[2] = members, info[3] as
 *   above (4: info[0] > out_cap, out is incomplete). out_cap >= rd_gz_grouped_out_bound(text_bytes, K) is always enough.
 * workspace [dev, 256-byte aligned] of rd_group_workspace_bytes(n, text_bytes, K, gz) bytes (gz != 0: rd_gz_compress_grouped's; 0:
 * bad arguments). Its largest piece under gz is the padded stream in front of the deflate, in which every key's run starts a member:
 * text_bytes + 65,280 * min(K, n) bytes at most, and 65,536 bytes of member slot per 65,280 of them. The counters of the partition are
 * 32-bit words in LDS up to K = 4,096 and words in the workspace beyond. n == 0: info and key_tab are zeroed. Asynchronous on `stream`. */
#define RD_SPLIT_GROUPS_MAX 1024
#define RD_GROUP_KEYS_MAX 16384
RD_API int rd_group_keys(const int32_t *rows, int64_t first, int64_t stride, int32_t mate, const int8_t *labels, int64_t n, const int32_t *class_slot,
                         int32_t G, int32_t *keys, int64_t *info, void *stream);
RD_API size_t rd_group_workspace_bytes(int64_t n, int64_t text_bytes, int32_t K, int32_t gz);
RD_API size_t rd_gz_grouped_out_bound(int64_t text_bytes, int32_t K);
RD_API int rd_group_pack(const uint8_t *text, int64_t text_bytes, const int64_t *rec_start, const int32_t *keys, int64_t n, int32_t K, uint8_t *out,
                         size_t out_cap, int64_t *key_tab, int64_t *info, void *workspace, size_t workspace_bytes, void *stream);
RD_API int rd_gz_compress_grouped(const uint8_t *text, int64_t text_bytes, const int64_t *rec_start, const int32_t *keys, int64_t n, int32_t K, uint8_t *out,
                                  size_t out_cap, int64_t *key_tab, int64_t *info, void *workspace, size_t workspace_bytes, void *stream);

/* The per-read report of a chunk (the CLI's --read_report) as ONE contiguous text in `out` [dev, 16-byte aligned]: line i, in input order,
 * is `<id>\t<label>\t<p>\n` (logits_b NULL: single-end) or `<id>\t<label>\t<p_a>\t<p_b>\t<p_pair>\n` (pairs). id = the bytes of record i's
 * header after its leading '@' / '>' up to the first of {space, \t, \r, \n, \v, \f} (may be empty); label = "rRNA" / "nonrRNA" /
 * "unclassified" for labels[i] = 1 / 0 / -1 (the labels that select the output files: rd_pair_fuse's, or rd_classify's uint8 labels);
 * p = softmax(logits)[1] of logits_a / logits_b [dev] fp32[n, 2], p_pair of their sum, in fp32 from d = l1 - l0, printed as
 * q = rint(p * 1e4): "0.dddd", "1.0000" when q = 10000. text / text_bytes / rec_start as rd_select_pack. line_start [dev] int64[n + 1]:
 * where line i starts (entry n = the report's bytes) - a record table of the report text, so that rd_gz_compress_selected deflates it
 * with an all-zero label vector and label 0. info [dev] int64[4]: info[0] = lines, info[1] = bytes written, info[3] != 0: nothing
 * written - 1: the report holds more than out_cap bytes, 2: a record does not start with '@' / '>', its header runs past rec_start[i + 1]
 * or its label is not -1 / 0 / 1. out_cap >= rd_report_out_bound(n, text_bytes) is always enough. Asynchronous on `stream`. */
RD_API size_t rd_report_workspace_bytes(int64_t n);
RD_API size_t rd_report_out_bound(int64_t n, int64_t text_bytes);
RD_API int rd_report_format(const uint8_t *text, int64_t text_bytes, const int64_t *rec_start, int64_t n, const float *logits_a, const float *logits_b,
                   const int8_t *labels, uint8_t *out, size_t out_cap, int64_t *line_start, int64_t *info, void *workspace, size_t workspace_bytes,
                   void *stream);

/* Paired-end reads from ONE interleaved FASTQ chunk (the CLI's --interleaved, an extension): records 2k and 2k + 1 of the chunk's 2n
 * records are mate 1 and mate 2 of pair k. text / text_bytes / rec_start [dev] int64[2n + 1] as rd_select_pack; seq_off [dev] int64[2n] and
 * seq_len [dev] int32[2n] as rd_classify takes them. rd_pair_split writes pair_start [dev] int64[n + 1] = rec_start[2k] (entry n = the
 * end): a pair is eight contiguous lines, so the pairs are the records of THIS table for rd_select_pack, rd_gz_compress_selected and
 * rd_report_format; and the mates' sequence tables seq_off1 / seq_len1 / seq_off2 / seq_len2 [dev, n entries each], contiguous arrays
 * for two rd_classify calls over the one text. check_ids != 0: the mate check - the id of a record is the bytes of its header after '@'
 * up to the first of {space, \t, \r, \n, \v, \f} (rd_report_format's); two records are mates when their ids are equal, or mate 1's ends
 * in "/1", mate 2's in "/2" and they are equal in front of those two bytes. info [dev] int64[4]: info[0] = pairs processed, info[1] =
 * index of the first pair whose ids are not mates or -1, info[3] != 0: nothing is to be trusted - a table entry lies outside the text
 * or, under check_ids, a record does not start with '@' or its header line runs past the record (check_ids == 0 reads no text).
 * No workspace; asynchronous on `stream`.
 * rd_pair_expand_labels: rec_labels [dev] int8[2n], rec_labels[2k + mate] = pair_labels[k] (mate 0 / 1) and the other mate's entry =
 * RD_LABEL_SKIP, a value no output file selects: the records of ONE mate by label are then rd_select_pack / rd_gz_compress_selected over
 * the full 2n-record table (they, and librd_host.so's rd_writer_write_selected, test labels for equality only). */
#define RD_LABEL_SKIP 2
RD_API int rd_pair_split(const uint8_t *text, int64_t text_bytes, const int64_t *rec_start, const int64_t *seq_off, const int32_t *seq_len, int64_t n_pairs,
                  int32_t check_ids, int64_t *pair_start, int64_t *seq_off1, int32_t *seq_len1, int64_t *seq_off2, int32_t *seq_len2, int64_t *info,
                  void *stream);
RD_API int rd_pair_expand_labels(const int8_t *pair_labels, int64_t n_pairs, int32_t mate, int8_t *rec_labels, void *stream);

/* The QC counters of a run (the CLI's --summary, an extension), accumulated where a chunk's text, sequence tables, final logits and
 * labels already are. acc [dev] int64[RD_SUM_WORDS], zeroed by the caller at run start; every call ADDS the counters of its chunk, so
 * the result is exact and does not depend on how the run was cut into chunks, shards or ranks (sum the ranks' arrays). A unit is a read
 * (text_b == NULL: single-end, mate 0 only) or a pair; class c = label + 1 (0 unclassified, 1 nonrRNA, 2 rRNA) of the UNIT; mate m = 0 / 1.
 *   RD_SUM_UNITS        [3]          units per label
 *   RD_SUM_MATE_LABELS  [3][2][2]    pairs by class and (argmax of mate 1's logits, of mate 2's); argmax = l1 > l0 (a tie: 0)
 *   RD_SUM_LENGTH       [2][3][513]  reads by mate, class and min(seq_len, 512) - the whole read, not the -l truncation
 *   RD_SUM_P_RRNA       [3][3][100]  source (mate 1, mate 2, the pair's summed logits) x class x bin; bin = min(q / 100, 99) with
 *                                    q = rint(softmax(logits)[1] * 1e4) in fp32, the value rd_report_format prints
 *   RD_SUM_BASES        [2][3][5]    bases of the whole read by code: A, C, G, T (with U), other (lowercase included)
 *   RD_SUM_GC           [2][3][101]  reads by 100 * (C + G) / (A + C + G + T), integer division; no A/C/G/T base: no bin
 * text_x / bytes_x / seq_off_x [dev] int64[n] / seq_len_x [dev] int32[n] as rd_classify takes them (the two mates may share one text);
 * logits_x [dev] fp32[n][2]; labels [dev] int8[n] in {-1, 0, 1}. info [dev] int64[4]: info[0] != 0 = NOTHING was added - a label outside
 * -1..1 (bit 0), a seq_len < 0 (bit 1) or a sequence that does not lie inside its text (bit 2); else info[1] = n. A check pass decides
 * that before the accumulate pass reads a byte. n == 0: a no-op (info, when given, is zeroed). Asynchronous on `stream`. */
#define RD_SUM_LEN_BINS 513
#define RD_SUM_P_BINS 100
#define RD_SUM_GC_BINS 101
#define RD_SUM_UNITS 0
#define RD_SUM_MATE_LABELS 3
#define RD_SUM_LENGTH 15
#define RD_SUM_P_RRNA 3093
#define RD_SUM_BASES 3993
#define RD_SUM_GC 4023
#define RD_SUM_WORDS 4629
RD_API int64_t rd_summary_words(void);
RD_API int rd_summary_accumulate(const uint8_t *text_a, int64_t bytes_a, const int64_t *seq_off_a, const int32_t *seq_len_a, const float *logits_a,
                          const uint8_t *text_b, int64_t bytes_b, const int64_t *seq_off_b, const int32_t *seq_len_b, const float *logits_b,
                          const int8_t *labels, int64_t n, int64_t *acc, int64_t *info, void *stream);

/* The optional fields (tags) of raw BAM records, and counters per read group (the CLI's --read_groups, an extension). The rule is
 * ribodetector_amd/bam.py (find_tag, group_row). raw [dev] uint8[raw_bytes] / raw_start [dev] int64[n_rec + 1]: a raw view as
 * rd_bam_raw_gather writes it - record k is raw[raw_start[k] .. raw_start[k + 1]), its block_size field first.
 * rd_bam_tag_find: for every record the first tag `tag` [host, 2 bytes]: val_off [dev] int64[n_rec] = where its value starts in raw
 * (-1: the record has no such tag; -2: its tags are malformed in front of or at the tag, or the record does not lie inside the view),
 * val_len [dev] int32[n_rec] = the value's bytes (Z / H: without the NUL; B: subtype and count included), val_type [dev] uint8[n_rec] =
 * the type byte; both 0 where val_off < 0. Every length in a record is data: it is checked against the record's end before a byte it
 * points to is read, and no byte outside [raw_start[k], raw_start[k + 1]) is read for record k.
 * rd_bam_group_rows: rows [dev] int32[n_rec] from the three tables of a search for "RG" and the dictionary of the G declared ids
 * (0 <= G <= RD_GROUPS_MAX), SORTED as unsigned bytes with a prefix in front of what it is a prefix of: dict_bytes [dev] the ids behind
 * one another (no id holds a NUL byte), dict_off [dev] int32[G + 1] where each starts. Row j: a Z value equal to id j; G: no tag; G + 1: a Z value that is no
 * declared id; G + 2: malformed tags or a tag that is not of type Z.
 * rd_bam_group_accumulate: acc [dev] int64[(G + 3) * 6 + 1], zeroed by the caller at run start, += the n units of a chunk. Unit u is
 * record first_a + stride_a * u of mate 1's view (and first_b + stride_b * u of mate 2's; raw_b == NULL: single-end; the two mates may
 * share one view). With g = rows_a[...] and class c = labels[u] + 1: acc[(g * 3 + c) * 2] += 1, acc[(g * 3 + c) * 2 + 1] += l_seq of
 * mate 1 (+ l_seq of mate 2), read from the raw records; acc[(G + 3) * 6] += 1 for a pair whose rows_b differs from g. info [dev]
 * int64[4]: info[0] != 0 = NOTHING was added - a label outside -1..1 (bit 0) or a row outside 0..G + 2 (bit 1); else info[1] = n. A
 * check pass decides that before the accumulate pass reads a record. n == 0: a no-op (info, when given, is zeroed). Integer sums: exact,
 * independent of the chunking. All three are asynchronous on `stream`. */
#define RD_GROUPS_MAX 65536
RD_API int rd_bam_tag_find(const uint8_t *raw, int64_t raw_bytes, const int64_t *raw_start, int64_t n_rec, const uint8_t *tag, int64_t *val_off,
                           int32_t *val_len, uint8_t *val_type, void *stream);
RD_API int rd_bam_group_rows(const uint8_t *raw, const int64_t *val_off, const int32_t *val_len, const uint8_t *val_type, int64_t n_rec,
                             const uint8_t *dict_bytes, const int32_t *dict_off, int32_t G, int32_t *rows, void *stream);
RD_API int rd_bam_group_accumulate(const uint8_t *raw_a, const int64_t *raw_start_a, const int32_t *rows_a, int64_t first_a, int64_t stride_a,
                                   const uint8_t *raw_b, const int64_t *raw_start_b, const int32_t *rows_b, int64_t first_b, int64_t stride_b,
                                   const int8_t *labels, int64_t n, int32_t G, int64_t *acc, int64_t *info, void *stream);

/* The listed tags of raw BAM records as text behind the read names of the records' FASTQ text (the CLI's --bam_tags, an extension).
 * The rule is ribodetector_amd/bam.py (tag_comment, fastq_text_tagged). text / rec_start: the FASTQ view of n_rec records (record k is
 * text[rec_start[k] .. rec_start[k + 1]), '@name\n...'); raw / raw_start: the raw view of the SAME records. tags [host]: n_tags names
 * of 2 bytes each ([A-Za-z][A-Za-z0-9], no name twice, 1 <= n_tags <= RD_BAM_TAGS_MAX). Record k of the tagged text is '@name', then
 * '\tTG:T:text' for every listed tag, in list order, that rd_bam_tag_find finds in raw record k, then the rest of the record from its
 * first '\n' on. A: TG:A:c; c C s S i I: TG:i:decimal; Z H: the bytes verbatim; B with an integer subtype s: TG:B:s and ',v' per
 * element. Values of type f and B:f are left out and counted. A record gets NO comment and is counted as malformed when a listed tag's
 * walk is malformed, an A / Z / H value holds a byte outside 0x20..0x7E, or an H value has odd length or a character that is no hex digit.
 * out [dev, 16-byte aligned] uint8[out_cap] receives the tagged text, out_start [dev] int64[n_rec + 1] its record table. info [dev]
 * int64[8 + RD_BAM_TAGS_MAX]: info[0] = records, info[1] = bytes of the tagged text, info[3] = fault - 1: the text needs more than
 * out_cap bytes (info[1] says how many; nothing in out is written, the counters are valid), 2: nothing is to be trusted (a table entry
 * outside its view, a FASTQ record that does not start with '@', a header line that runs past its record); info[4] = records with
 * malformed tags, info[5] = float values skipped, info[8 + j] = records in which tag j was copied. The tagged text has no bound linear
 * in text_bytes (text_bytes + 5 raw_bytes always holds it): a caller sizes out by a hint and repeats once on fault 1.
 * workspace [dev, 256-byte aligned] of rd_bam_tag_splice_workspace_bytes(n_rec, n_tags) (0: bad arguments). Every length read from raw
 * is checked against the record's end before the byte it points to is read (rd_bam_tag_find's contract). Asynchronous on `stream`;
 * n_rec == 0: a no-op that zeroes info. */
#define RD_BAM_TAGS_MAX 16
RD_API size_t rd_bam_tag_splice_workspace_bytes(int64_t n_rec, int32_t n_tags);
RD_API int rd_bam_tag_splice(const uint8_t *text, int64_t text_bytes, const int64_t *rec_start, const uint8_t *raw, int64_t raw_bytes,
                             const int64_t *raw_start, int64_t n_rec, const uint8_t *tags, int32_t n_tags, uint8_t *out, size_t out_cap,
                             int64_t *out_start, int64_t *info, void *workspace, size_t workspace_bytes, void *stream);

/* rd_bam_tag_splice with flags (the CLI's --bam_tag_floats): rd_bam_tag_splice is this call with flags = 0. A flag bit that is not
 * listed here is RD_E_INVALID (nothing is launched). RD_BAM_TAGS_FLOATS: a listed tag of type f becomes 'TG:f:text', a B array with
 * subtype f 'TG:B:f' and ',text' per element (none: 'TG:B:f' alone), text = the value as rd_float_text writes it; such a tag counts as
 * copied (info[8 + j]) and info[5] is 0. An f value whose length is not 4 makes the record malformed, as for the integer types. info
 * keeps its layout, the workspace is that of rd_bam_tag_splice_workspace_bytes, and text_bytes + 5 raw_bytes still holds the tagged
 * text (an element of 4 bytes prints as at most 13).
 * rd_float_text: the float32 values with the bit patterns bits [dev] uint32[n] as text, the rule of ribodetector_amd/bam.py (float_g):
 * what printf("%g", (double)v) prints - the EXACT value m 2^e rounded to 6 significant decimal digits, ties to even, in fixed form when
 * the decimal exponent after rounding is in -4..5, else d.ddddde+XX, trailing zeros removed; inf, nan, 0; '-' in front when the sign bit
 * is set (-0, -inf and -nan included). Value k: text [dev, 16-byte aligned] uint8[16 n] bytes [16 k, 16 k + len[k]), the slot of 16 bytes
 * written whole by one store (zero behind the text); len [dev] uint8[n], 1..12. Integer arithmetic throughout, no double (csrc/
 * rd_float_text.hpp). n == 0: a no-op; a null pointer: RD_E_INVALID. Asynchronous on `stream`. */
#define RD_BAM_TAGS_FLOATS 1u
RD_API int rd_bam_tag_splice_ex(const uint8_t *text, int64_t text_bytes, const int64_t *rec_start, const uint8_t *raw, int64_t raw_bytes,
                                const int64_t *raw_start, int64_t n_rec, const uint8_t *tags, int32_t n_tags, uint8_t *out, size_t out_cap,
                                int64_t *out_start, int64_t *info, void *workspace, size_t workspace_bytes, uint32_t flags, void *stream);
RD_API int rd_float_text(const uint32_t *bits, int64_t n, uint8_t *text, uint8_t *len, void *stream);

/* The records of a FASTQ / FASTA chunk as unaligned BAM records (CLI extension `--ubam_output`; csrc/rd_bam_encode.hpp): the raw view
 * of a chunk that did not come from a BAM file. The rule is ribodetector_amd/bam.py (from_fastq). text / rec_start / seq_off / seq_len:
 * a chunk as rd_fastq_gather / rd_fasta_gather leave it. Record i = 0 .. n_rec - 1 of the call is entry rec_first + i * rec_stride of the
 * tables (rec_start is read at that entry and the one behind it; rec_first >= 0, rec_stride >= 1). flags: RD_UBAM_FASTA (the records
 * are '>' header '\n' SEQ '\n': qualities 0xFF) | the BAM flag word of the call's even records << RD_UBAM_EVEN_SHIFT | that of its odd
 * records << RD_UBAM_ODD_SHIFT (12 bits each) - 4 and 4: single-end; 77 and 77: mate 1's file; 141 and 141: mate 2's; 77 and 141: an
 * interleaved chunk. Any other bit: RD_E_INVALID. Record i becomes: block_size, refID -1, pos -1, l_read_name, mapq 0, bin 4680,
 * n_cigar_op 0, flag, l_seq, next_refID -1, next_pos -1, tlen 0; the name and a NUL; the bases, 4 bits each; the qualities; no tags.
 * name = the id of rd_report_format, without a trailing /1 (flag & 0x40) or /2 (flag & 0x80) when flag & 1; an empty one becomes '*'.
 * A base: the code of its letter in "=ACMGRSVTWYHKDBN", either case, U as T, any other byte 15. A quality: min(max(b, 33), 126) - 33.
 * raw [dev, 16-byte aligned] uint8[raw_cap] receives the records, raw_start [dev] int64[n_rec + 1] their table. raw_cap >=
 * text_bytes + 32 n_rec (FASTQ) or text_bytes + (text_bytes + 1) / 2 + 40 n_rec (FASTA) is always enough. info [dev] int64[8]:
 * [0] records, [1] raw bytes, [2] the first record (index in the call) whose name is longer than 254 bytes or -1 - it is laid out with
 * the first 254 -, [3] fault - 1: more than raw_cap bytes, 2: a table entry that does not describe the text; nothing is written into raw
 * then, raw_start is zeroed and [0] [1] are 0 -, [4] bytes whose BAM letter differs from the input byte, [5] quality bytes outside
 * 33..126, [6] names replaced by '*', [7] the first record whose quality line is not as long as its sequence or -1 (laid out with
 * l_seq 0). A caller delivers nothing of a call whose [2] or [7] is not -1. workspace [dev, 256-byte aligned] of
 * rd_bam_encode_workspace_bytes(n_rec) (0: bad n_rec). Every table entry is checked against text_bytes before it is followed and every
 * output offset against raw_cap. Asynchronous on `stream`; n_rec == 0: info = {0, 0, -1, 0, 0, 0, 0, -1}, raw_start[0] = 0. */
#define RD_UBAM_FASTA 1u
#define RD_UBAM_EVEN_SHIFT 4
#define RD_UBAM_ODD_SHIFT 16
RD_API size_t rd_bam_encode_workspace_bytes(int64_t n_rec);
RD_API int rd_bam_encode(const uint8_t *text, int64_t text_bytes, const int64_t *rec_start, const int64_t *seq_off, const int32_t *seq_len,
                         int64_t n_rec, int64_t rec_first, int32_t rec_stride, uint32_t flags, uint8_t *raw, size_t raw_cap,
                         int64_t *raw_start, int64_t *info, void *workspace, size_t workspace_bytes, void *stream);

/* rd_bam_encode with the tags of the header lines' comments (CLI extension `--ubam_tags`; the rule is bam.py tags_from_comment). names
 * [host]: n_names names of 2 bytes each ([A-Za-z][A-Za-z0-9], no name twice, 0 <= n_names <= RD_BAM_TAGS_MAX). n_names == 0 IS
 * rd_bam_encode: the same launches, info int64[8]. Else every record ends in the listed tags that its header line's comment holds, in
 * comment order, and block_size includes them. The header line ends in front of its '\n' (one '\r' in front of that is not part of it);
 * the comment is every byte behind the ONE byte that ends the id; it is split at '\t'; a field 'XY:T:value' (X a letter, Y a letter or
 * digit, T one of A i Z H B f) with a listed name counts when it is the first of its name. A: one byte 0x21..0x7E. i: [+-]?[0-9]{1,10}
 * in [-2^31, 2^32 - 1], stored in the smallest of C S I (v >= 0) / c s i. Z: bytes 0x20..0x7E, H: an even number of hex digits, both
 * with a NUL. B: a subtype of cCsSiI, then ',int' per element, each inside the subtype's range: subtype, count:uint32, elements. f and
 * B:f are left out and counted. Anything else makes the record malformed: it gets no tags and is counted once. info [dev]
 * int64[10 + n_names]: [0]..[7] as rd_bam_encode, but with fault 1 info[1] = the bytes the records need (a caller repeats the call
 * once at that size); [8] records with malformed tags, [9] float values skipped, [10 + j] records in which name j was copied. A
 * field of t text bytes makes at most max(t, 2 t - 4) tag bytes, so the bound of rd_bam_encode plus the comments' bytes always holds
 * the records, and real comments shrink. A header line without '\n' inside its record is fault 2. workspace of
 * rd_bam_encode_tags_workspace_bytes(n_rec, n_names) (n_names == 0: rd_bam_encode_workspace_bytes(n_rec)). Every offset the comment
 * walk follows is compared with the record's end before it is read.
 * flags | RD_UBAM_TAG_FLOATS (CLI extension `--ubam_tag_floats`; bit 28 - bits 0, 4..15 and 16..27 are taken): f and B:f values become
 * float32 tags instead of being left out. An f value is of the syntax of rd_float_parse -> XY f and its 4 bytes; a B:f value is 'f', then
 * ',value' per element ('XY:B:f' alone: none) -> XY B f count:uint32 and the elements. Such a tag counts as copied ([10 + j]). A value
 * or element that is not of the syntax, an empty element, a trailing comma or a byte behind 'f' that is no comma makes the record
 * malformed; a value, or any element, of more than 17 significant digits leaves the tag out and adds 1 to [9], which then counts
 * nothing else. info keeps its layout, the workspace its size, and an f field of t >= 6 text bytes makes 7, a B:f field of t >= 6 + 2 n
 * makes 8 + 4 n: the same bound. With n_names == 0, or passed to rd_bam_encode, the bit is RD_E_INVALID.
 * rd_float_parse: the texts of n float values as float32 bit patterns, the rule of ribodetector_amd/bam.py (float_from_text). Value k is
 * text [dev] bytes [start[k], start[k + 1]), start [dev] int64[n + 1]; every offset is compared with start[n] before it is read (an
 * entry outside 0 <= start[k] <= start[k + 1] <= start[n] gives status 1). Syntax: [+-]? ( D+ | D* '.' D+ ) ( [eE] [+-]? D{1,4} )? with
 * D = [0-9], or [+-]? inf / nan in any letter case. bits [dev] uint32[n]: inf 0x7f800000, nan 0x7fc00000, the sign bit for '-'; else, with
 * M the digits without their leading and trailing zeros and v = M 10^q the EXACT value, the float32 nearest to v, ties to the even
 * mantissa, denormals included, in one rounding (v >= 2^128 - 2^103: infinity; v <= 2^-150: zero). status [dev] uint8[n]: 0 converted,
 * 1 not of the syntax, 2 more than 17 significant digits (bits is 0 for 1 and 2). Integer arithmetic, no double (csrc/
 * rd_float_parse.hpp). One lane per value. n == 0: a no-op; a null pointer: RD_E_INVALID. Asynchronous on `stream`. */
#define RD_UBAM_TAG_FLOATS (1u << 28)
RD_API int rd_float_parse(const uint8_t *text, const int64_t *start, int64_t n, uint32_t *bits, uint8_t *status, void *stream);
RD_API size_t rd_bam_encode_tags_workspace_bytes(int64_t n_rec, int32_t n_names);
RD_API int rd_bam_encode_ex(const uint8_t *text, int64_t text_bytes, const int64_t *rec_start, const int64_t *seq_off, const int32_t *seq_len,
                            int64_t n_rec, int64_t rec_first, int32_t rec_stride, uint32_t flags, const uint8_t *names, int32_t n_names,
                            uint8_t *raw, size_t raw_cap, int64_t *raw_start, int64_t *info, void *workspace, size_t workspace_bytes,
                            void *stream);

/* Reads longer than max_len classified over WINDOWS of max_len bases (CLI extension `--windows`; the reference classifies read[:max_len],
 * reference detect.py:666-726, and that stays the rule without the flag). A window is one more (seq_off, seq_len) entry over the same
 * text, so rd_classify takes the window table as it takes a read table and its kernels do not change.
 * The rule, with L = max_len, S = stride (1..2^31-1), K = max_windows (1..RD_WINDOW_MAX): a read of len bases has W = 1 window when
 * len <= L, else W = min(K, ceil((len - L) / S) + 1). W == 1: the window is the read's own entry (seq_off, seq_len), unchanged - rd_classify
 * truncates it as ever, the logits are those of the read. W > 1: window j = 0..W-1 starts at seq_off + (j (len - L)) / (W - 1) (integer
 * division in int64) and has L bases: the first at the read's start, the last at its end, no short tail window.
 * rd_window_plan: win_first [dev] int64[n + 1] = the exclusive scan of W (entry n = the total). info [dev] int64[4] = {n, total windows,
 * 0, fault}: fault != 0 = a seq_len < 0, nothing is to be trusted. workspace [dev, 256-byte aligned] of rd_window_workspace_bytes(n).
 * rd_window_fill: win_off [dev] int64[total] / win_len [dev] int32[total], the window table, from the same integers (total: info[1] of
 * the plan, read back by the caller - it sizes the table; entries outside [0, total) are never written). It reads no text.
 * rd_window_fuse: win_logits [dev, 8-byte aligned] fp32[total][2] (rd_classify over the window table, FINAL: after rd_sync_results under
 * rd_set_refine_async) -> logits [dev, 8-byte aligned] fp32[n][2] and labels [dev] uint8[n] (or NULL) = logits[1] > logits[0].
 * RD_WINDOW_MEAN: ((w_0 + w_1) + w_2 + ...) / (float)W per class, a sequential fp32 sum in window order and one correctly rounded division
 * (W == 1: w_0 bit for bit). RD_WINDOW_MAX_D: the logits of the window with the largest d = w[1] - w[0] (fp32), the lowest window on a tie.
 * only_multi != 0: rows with W == 1 (logits and labels) are left as they are. Every window's logits carry rd_classify's guarantees (the
 * float64 pass included); a FUSED margin inside the fp32 noise band has no float64 guarantee. n == 0: no-ops (the plan zeroes info and
 * win_first[0]). Asynchronous on `stream`. */
#define RD_WINDOW_MAX 4096
#define RD_WINDOW_MEAN 0
#define RD_WINDOW_MAX_D 1
RD_API size_t rd_window_workspace_bytes(int64_t n);
RD_API int rd_window_plan(const int32_t *seq_len, int64_t n, int32_t max_len, int64_t stride, int32_t max_windows, int64_t *win_first, int64_t *info,
                   void *workspace, size_t workspace_bytes, void *stream);
RD_API int rd_window_fill(const int64_t *seq_off, const int32_t *seq_len, const int64_t *win_first, int64_t n, int32_t max_len, int64_t stride,
                   int32_t max_windows, int64_t total, int64_t *win_off, int32_t *win_len, void *stream);
RD_API int rd_window_fuse(const float *win_logits, const int64_t *win_first, int64_t n, int32_t mode, int32_t only_multi, float *logits, uint8_t *labels,
                   void *stream);

/* WHERE the rRNA is inside reads classified over windows (CLI extension `--regions`, with `--windows`): one text line per REGION of a
 * chunk, made where the windows' final logits, the reads' lengths and the records' text already are. A unit is a read (text_b == NULL:
 * single-end) or one mate of a pair; x_a are mate 1's tables, x_b mate 2's (the mates may share one text). Per mate: text_x [dev] /
 * bytes_x; rec_start_x [dev] int64: record i starts at rec_start_x[i * rec_stride] and ends at the next entry (rec_stride 1: a table of
 * n + 1 entries per mate; 2: an interleaved chunk's table of 2 n + 1 entries, rec_start_b = rec_start_a + 1); seq_len_x [dev] int32[n];
 * win_first_x [dev] int64[n + 1] of rd_window_plan; win_logits_x [dev, 8-byte aligned] fp32[win_first_x[n]][2], FINAL (rd_sync_results).
 * The rule, L = max_len: window j of a read is an rRNA window when l1 > l0 (a tie is not); it covers [start(j), start(j) + L) with
 * start(j) = (j (len - L)) / (W - 1) of rd_window_fill when W > 1, [0, min(len, L)) when W == 1. A region is a maximal run a..b of rRNA
 * windows of one read = [start(a), start(b) + L) in 0-based bases of the read (the unsampled bases between two rRNA windows belong to
 * it; with a stride below L / 2 two regions may overlap); a region of no bases has no line. The line:
 * `<id>\t<start>\t<end>\t<mate>\t<windows>\t<p_rrna_max>\n`, id as rd_report_format's (of THAT mate's record), start / end decimal, mate
 * 1 / 2, windows = b - a + 1, p_rrna_max = the largest q = rint(softmax(logits)[1] * 1e4) of the run's windows as rd_report_format
 * prints it. Order: units in input order, mate 1's lines before mate 2's, ascending start within a read. No header line is written.
 * out [dev, 16-byte aligned] of out_cap bytes: the text has no bound linear in the text bytes (an id is repeated per region), so the
 * caller guesses and repeats on fault 1. info [dev] int64[8] = {units, bytes, 0, fault, regions of mate 1, of mate 2, reads of mate 1
 * with a region, of mate 2}. fault 1: the lines need info[1] > out_cap bytes, nothing is written (info[4..8) are valid). fault 2: a
 * table entry outside its text, a header that does not start with '@' / '>' or runs past its record, a seq_len < 0, a win_first that is
 * not increasing by 1..RD_WINDOW_MAX per read inside [0, win_first[n]], several windows on a read of at most L bases, or more windows
 * than the workspace was sized for: nothing is written, info[0], info[1], info[4..8) = 0. workspace [dev, 256-byte aligned] of
 * rd_region_workspace_bytes(n, total windows of both mates). n == 0: a no-op that zeroes info. Asynchronous on `stream`. */
RD_API size_t rd_region_workspace_bytes(int64_t n, int64_t total_windows);
RD_API int rd_region_format(const uint8_t *text_a, int64_t bytes_a, const int64_t *rec_start_a, const int32_t *seq_len_a, const int64_t *win_first_a,
                     const float *win_logits_a, const uint8_t *text_b, int64_t bytes_b, const int64_t *rec_start_b, const int32_t *seq_len_b,
                     const int64_t *win_first_b, const float *win_logits_b, int64_t rec_stride, int64_t n, int32_t max_len, uint8_t *out, size_t out_cap,
                     int64_t *info, void *workspace, size_t workspace_bytes, void *stream);

/* ONE DEFLATE stream - a plain .gz, the format sequencers write - inflated on the device (round 5; the CLI's default for such FASTQ, RD_DEVICE_INFLATE=members keeps the host's decoders).
 * Replaces, for such files: gzip.open(path, 'rt') of reference data_loader/seq_encoder.py:21-39. The two-pass scheme of pugz (this
 * build's host reader: csrc/rd_pgzip.h) with one wave per SECTION of `section_bytes` compressed bytes: block starts are searched on the
 * device, every section is decoded from its start to the next section's start with an unknown window into 16-bit symbols, the windows
 * are resolved in order and all sections in parallel. The stream arrives in batches:
 *   comp [dev, 4-byte aligned] holds `valid_bytes` bytes of the file from the batch's first byte (comp_bytes readable); the sections
 *   cover [0, data_bytes) and one more section behind them is searched for the start the NEXT batch begins with (so valid_bytes >=
 *   data_bytes + section_bytes unless the file ends; the next batch's buffer starts `data_bytes` further: carry_delta_bits =
 *   8 * data_bytes). first_start_bit: where the member's first block starts (first batch: behind the gzip header; else ignored and taken
 *   from `carry` = the state the batch before left [dev]). win_in / win_out [dev] 32 KiB: the text behind the batch before / this one.
 *   text [dev, 8-byte aligned] receives state->n_text bytes (<= text_cap). state [dev] rd_gzs_state: status RD_GZS_* (MISMATCH: a section did not
 *   end where the next one starts - nothing speculative is ever accepted; OVERFLOW: a section made more than cap_syms symbols; ...),
 *   final: the member ended in this batch at bit `end_bit` of comp (its trailer - CRC-32, ISIZE - follows at the next byte boundary: the
 *   caller compares them with state->crc and total_len). Asynchronous on `stream`. */
typedef struct rd_gzs_state {
    uint64_t total_len;
    int64_t n_text;
    uint32_t crc, status, final, end_bit, next_start, win_valid, bad_section, n_sections;
    uint64_t reserved[2];
} rd_gzs_state;
#define RD_GZS_OK 0
#define RD_GZS_DECODE 1
#define RD_GZS_MISMATCH 2
#define RD_GZS_OVERFLOW 3
#define RD_GZS_NOSTOP 4
#define RD_GZS_WINDOW 5
#define RD_GZS_TEXTCAP 6
#define RD_GZS_NOSTART 7
RD_API size_t rd_gz_stream_workspace_bytes(int64_t data_bytes, int32_t section_bytes, int32_t cap_syms, int64_t text_cap);
RD_API int rd_gz_stream_inflate(const uint8_t *comp, int64_t comp_bytes, int64_t data_bytes, int64_t valid_bytes, int32_t section_bytes, int32_t cap_syms,
                         uint32_t first_start_bit, const rd_gzs_state *carry, int64_t carry_delta_bits, int32_t at_eof, const uint8_t *win_in,
                         uint8_t *win_out, uint8_t *text, int64_t text_cap, rd_gzs_state *state, void *workspace, size_t workspace_bytes, void *stream);

/* Round 6 - a RANGE of such a stream decoded before the text in front of it is known: what lets the ranks of a node share ONE .gz
 * (rank r decodes the compressed bytes [r S / W, (r + 1) S / W) on its own GPU while rank r - 1 still decodes its share). Replaces, for W > 1,
 * the same gzip.open(path, 'rt') of reference data_loader/seq_encoder.py:21-39,75-87 that every rank would otherwise repeat (or one rank
 * perform for all). rd_gz_range_decode is rd_gz_stream_inflate up to the window chain, which runs on SYMBOLS: sym_text [dev, 16-byte
 * aligned] receives state->n_text 16-bit symbols - a byte, or 0x8000 | i = "byte i of the 32 KiB in front of the RANGE" - and map_out [dev]
 * uint16[32768] the 32 KiB behind the batch in the same form: the range's MAP so far. Batches of a range chain through carry / map_in (both
 * null for its first batch). first_start_bit = RD_GZS_SEARCH: the range starts inside the stream, its first block start is searched like
 * every section's (state->reserved[0] = the bit found: it must equal the next_start the range before reports, nothing speculative is
 * accepted); a rank whose range holds the gzip header passes the bit behind it. state: as above, crc / total_len / win_valid untouched.
 * The ranks exchange their maps, apply them in rank order on the host (window[r + 1][i] = map[r][i] is a byte ? it : window[r][map[r][i] &
 * 0x7fff]) and call rd_gz_range_resolve per batch: text [dev, 16-byte aligned] = the n symbols as bytes, window [dev] uint8[32768] the
 * 32 KiB in front of the range of which the LAST win_valid bytes are text of the member (a marker in front of them: state->status =
 * RD_GZS_WINDOW); state [dev, zeroed by the caller before the range's first call] accumulates crc / total_len over the calls (CRC-32 of the
 * range's text alone: the ranks' values are combined like zlib's crc32_combine and compared with the member's trailer). */
#define RD_GZS_SEARCH 0xfffffffeu
RD_API size_t rd_gz_range_workspace_bytes(int64_t data_bytes, int32_t section_bytes, int32_t cap_syms, int64_t text_cap);
RD_API int rd_gz_range_decode(const uint8_t *comp, int64_t comp_bytes, int64_t data_bytes, int64_t valid_bytes, int32_t section_bytes, int32_t cap_syms,
                       uint32_t first_start_bit, const rd_gzs_state *carry, int64_t carry_delta_bits, int32_t at_eof, const uint16_t *map_in, uint16_t *map_out,
                       uint16_t *sym_text, int64_t text_cap, rd_gzs_state *state, void *workspace, size_t workspace_bytes, void *stream);
RD_API size_t rd_gz_range_resolve_workspace_bytes(int64_t n);
RD_API int rd_gz_range_resolve(const uint16_t *sym_text, int64_t n, const uint8_t *window, uint32_t win_valid, uint8_t *text, rd_gzs_state *state, void *workspace,
                        size_t workspace_bytes, void *stream);

/* n bytes moved by a kernel on `stream` instead of a DMA engine: dst / src [dev, or pinned host memory mapped into the device]. The
 * feeder's H2D of file bytes and the writers' D2H of output bytes use it: an SDMA queue is shared in order with other streams' copies,
 * and a copy that waits for kernels (a label D2H behind two recurrence launches) held a 96 MB H2D back for 60-100 ms. workgroups (of 1,024 threads): 0 = 8 - few and fat, because a
 * workgroup that copies keeps its CU from the recurrence kernel for as long as the copy runs. */
RD_API int rd_copy_bytes(void *dst, const void *src, int64_t n, int32_t workgroups, void *stream);

/* A HIP stream whose kernels run on a subset of the compute units (hipExtStreamCreateWithCUMask): cu_mask [host] uint32[words], bit i =
 * CU i may be used (MI355X: 256 CUs = 8 words; the driver spreads consecutive bits over the XCDs). words == 0: an ordinary stream,
 * priority < 0 = the device's highest. Why: the latency-bound side kernels (inflate, FASTQ index, deflate) otherwise queue behind a
 * recurrence launch that holds every register file for ~30 ms; on CUs of their own they run beside it. The caller
 * wraps the handle (torch.cuda.ExternalStream) and destroys it when done. */
RD_API int rd_stream_create(int device, const uint32_t *cu_mask, int words, int priority, void **stream);
RD_API int rd_stream_destroy(void *stream);

/* Timing of the dominant kernel, for bench.py's roofline: rd_classify records hipEvents around the recurrence
 * kernel on the launch stream when enabled. rd_profile_read synchronises those events and returns the number of
 * recorded launches and their total duration. */
RD_API int rd_profile_enable(rd_model *m, int enable);
RD_API int rd_profile_read(rd_model *m, int64_t *launches, double *total_ms);

RD_API const char *rd_last_error(void);
RD_API const char *rd_version(void);

#ifdef __cplusplus
}
#endif
#endif /* RIBODETECTOR_AMD_H */
