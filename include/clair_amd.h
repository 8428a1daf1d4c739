/*
 * clair_amd.h -- C ABI of the MI355X (gfx950) engine for Clair's call_var forward pass.
 *
 * The reference has no FFI: its boundary for this path is the Python class
 * clair.model.Clair (/root/reference/clair/model.py:24) as driven by
 * clair/call_var.py:213-215, 1337, 1343.  Each entry point below names the reference
 * member it stands behind; clair_amd/model.py is the ctypes shim that re-creates the
 * Python interface on top of it (INTEGRATION.md shows the binding).
 *
 * Conventions: plain pointers and sizes only; every function returns 0 on success and a
 * non-zero code on failure, with a message available from clair_last_error(); float32
 * everywhere (clair/model.py:167-168 forces tf.float32 for the LSTM structure).
 * Functions taking an engine are not re-entrant on one engine (the reference never calls
 * predict concurrently with itself, clair/call_var.py:1349-1352) but may be called from
 * any thread: the HIP device is selected on every call.
 */
#ifndef CLAIR_AMD_H
#define CLAIR_AMD_H

#include <stdint.h>
#include "clair_call.h"

#ifdef __cplusplus
extern "C" {
#endif

/* 1: round-1 surface.  2: + clair_slot_input, clair_submit_counts, clair_kernel_workgroups (added late in round 1 without a
 * bump), the clair_comm_* communicator (round 2).  3: + clair_engine_counter, clair_comm_preflight, clair_submit_ex, clair_decode, clair_pinned_alloc / _free and kernel id CLAIR_K_DECODE (round 3).
 * 4: + the clair_frontend_* device front end; clair_submit_ex takes device pointers (round 3).
 * 5: + clair_device_pci_bus_id (round 5: a rank finds the NUMA node of ITS GPU, clair_amd/shard.py), clair_comm_abort.
 * 6: + clair_comm_create_timed (round 6: a hung RCCL bring-up ends at a deadline, not at the job's). */
#define CLAIR_ABI_VERSION 6

/* geometry: shared/param.py:9-11 (33 x 8 x 4 input), clair/task/main.py:10-29 (head sizes) */
#define CLAIR_POSITIONS 33
#define CLAIR_FEATURES 32
#define CLAIR_INPUT_FLOATS (CLAIR_POSITIONS * CLAIR_FEATURES) /* 1056 */
#define CLAIR_GT21 21
#define CLAIR_GENOTYPE 3
#define CLAIR_INDEL_LEN 33
#define CLAIR_OUTPUT_FLOATS 90

/* Weight tensors of the inference graph (clair/model.py:400-620), row-major, float32.
 * TF variable names: clair_amd/weights.py:tf_variable_names(). */
enum clair_tensor_id {
    CLAIR_T_LSTM1_FW_KERNEL = 0, /* [160,512]  rows 0..31 multiply x, 32..159 multiply h; cols i|c~|f|o */
    CLAIR_T_LSTM1_FW_BIAS = 1,   /* [512] */
    CLAIR_T_LSTM1_BW_KERNEL = 2,
    CLAIR_T_LSTM1_BW_BIAS = 3,
    CLAIR_T_LSTM2_FW_KERNEL = 4, /* [384,512] */
    CLAIR_T_LSTM2_FW_BIAS = 5,
    CLAIR_T_LSTM2_BW_KERNEL = 6,
    CLAIR_T_LSTM2_BW_BIAS = 7,
    CLAIR_T_L3_KERNEL = 8,       /* [256,33,30]  L3/Unit_c/kernel stacked over c */
    CLAIR_T_L3_BIAS = 9,         /* [256,30] */
    CLAIR_T_L4_KERNEL = 10,      /* [7680,192]  input index u*256+c */
    CLAIR_T_L4_BIAS = 11,        /* [192] */
    CLAIR_T_L5_KERNEL = 12,      /* [4,192,96]  L5_1..L5_4 */
    CLAIR_T_L5_BIAS = 13,        /* [4,96] */
    CLAIR_T_HEAD_GT21_KERNEL = 14,     /* [96,21] */
    CLAIR_T_HEAD_GT21_BIAS = 15,
    CLAIR_T_HEAD_GENOTYPE_KERNEL = 16, /* [96,3] */
    CLAIR_T_HEAD_GENOTYPE_BIAS = 17,
    CLAIR_T_HEAD_LEN1_KERNEL = 18,     /* [96,33] */
    CLAIR_T_HEAD_LEN1_BIAS = 19,
    CLAIR_T_HEAD_LEN2_KERNEL = 20,     /* [96,33] */
    CLAIR_T_HEAD_LEN2_BIAS = 21,
    CLAIR_T_COUNT = 22
};

/* kernels of one forward pass, in launch order (index into clair_kernel_times) */
enum clair_kernel_id {
    CLAIR_K_PROJ1 = 0,  /* (unused since the LSTM1 input projection is fused into CLAIR_K_LSTM1) */
    CLAIR_K_LSTM1 = 1,  /* LSTM1: input projection + recurrence, both directions */
    CLAIR_K_PROJ2 = 2,  /* LSTM2 input projection GEMM  [33n,256]x[256,1024] */
    CLAIR_K_LSTM2 = 3,  /* LSTM2 recurrence                                  */
    CLAIR_K_L3 = 4,     /* (unused: slice dense is fused into CLAIR_K_L4)    */
    CLAIR_K_L4 = 5,     /* slice dense 256 x (33->30) + selu, split-K GEMM 7680->192 */
    CLAIR_K_TAIL = 6,   /* L4 reduce+selu, L5 x4, heads, selu, softmax       */
    CLAIR_K_DECODE = 7, /* probabilities -> call records (clair_submit_ex only) */
    CLAIR_K_COUNT = 8
};

typedef struct clair_engine clair_engine_t;

/* -- lifetime: Clair() + Clair.init()  (clair/model.py:58-192, 807-813) ------------------------
 * device: HIP device ordinal.  max_batch: largest n accepted by one predict/submit.
 * n_slots: submits that may be pending at once (clair_submit* .. clair_wait); 1 is enough for the synchronous predict.  A slot owns the
 * input and output buffers of its batch on both sides of the host link.  The forward passes themselves run on compute LANES (a HIP stream
 * + the inter-kernel workspaces each): one per slot up to four slots (the process has four hardware queues), three for a handle with more
 * slots (the fourth queue is the incoming copy stream's), slot s on lane s % lanes; with twice as
 * many slots as lanes a lane computes one batch of its slots while the copy engine brings the other one in, which is what takes the
 * host-array boundary from half of the HBM-resident rate to within a few per cent of it.  clair_run_resident(slot)
 * runs on the slot's lane. */
int clair_engine_create(int device, int max_batch, int n_slots, clair_engine_t **out);
/* Clair.close() / __del__  (clair/model.py:872-876, 1149-1152) */
void clair_engine_destroy(clair_engine_t *e);
/* message of the last failure on this engine (e may be NULL: failure of clair_engine_create) */
const char *clair_last_error(const clair_engine_t *e);
int clair_abi_version(void);
/* number of HIP devices visible (0 when there is none); negative never */
int clair_device_count(void);
/* "dddd:bb:dd.f" of HIP device `device` into buf (NUL-terminated; len >= 16): the name of its directory under
 * /sys/bus/pci/devices, where numa_node and local_cpulist say which host cores sit next to it.  The reference pins its
 * stages to cores with taskset (clair/callVarBam.py:103-115); a rank of this library pins itself to the cores of its GPU's
 * NUMA node (clair_amd/shard.py: bind_to_gpu).  0 on success; 1 when there is no such device (buf[0] = 0). */
int clair_device_pci_bus_id(int device, char *buf, int len);

/* -- weights: Clair.restore_parameters()  (clair/model.py:1016-1020) ----------------------------
 * Hand over one tensor (host pointer, `count` floats, shape as in enum clair_tensor_id);
 * after all CLAIR_T_COUNT tensors are set, clair_finalize_weights packs them into the
 * device layouts the kernels read.  The host pointers are not retained. */
int clair_set_tensor(clair_engine_t *e, int tensor_id, const float *host, int64_t count);
int clair_finalize_weights(clair_engine_t *e);

/* -- Clair.predict(batchX)  (clair/model.py:946-966; called at clair/call_var.py:1343) ----------
 * x: host, C-contiguous [n,33,8,4] float32 (channels 1..3 already minus channel 0,
 * clair/utils.py:96-98); 1 <= n <= max_batch.  Outputs: caller-allocated host arrays
 * [n,21] [n,3] [n,33] [n,33].  Synchronous; x is not retained. */
int clair_predict(clair_engine_t *e, const float *x, int n, float *gt21, float *genotype,
                  float *indel_len1, float *indel_len2);

/* -- pipelined form of the same call (what call_var's load/predict/output threads overlap,
 *    clair/call_var.py:1331-1352): submit copies x to the device and enqueues the forward pass on
 *    slot `slot`; wait blocks until that slot's outputs are in the caller's arrays.
 *    x and the output arrays must stay valid until wait returns. */
int clair_submit(clair_engine_t *e, int slot, const float *x, int n, float *gt21, float *genotype,
                 float *indel_len1, float *indel_len2);
/* (A batch in pageable memory is copied to the slot's page-locked buffer, and its transfers and kernels are enqueued, by a staging
 * thread of the engine: clair_submit returns at once and clair_wait reports a failure of that work.  This is why x must stay valid
 * until clair_wait, as the reference's predict thread leaves loading and output to two others, clair/call_var.py:1331-1352.) */
/* (clair_wait itself asks for no weights: every submit has checked what it needs, and clair_submit_site_calls needs none.  On a slot
 * with nothing pending it returns 0.) */
int clair_wait(clair_engine_t *e, int slot);
/* The slot's own page-locked input buffer, [max_batch][33][8][4] float32.  A producer that writes its batch there and passes
 * this pointer as `x` to clair_submit gets a direct DMA transfer (pageable memory goes through the runtime's staging copies at
 * about a third of the PCIe rate).  The buffer belongs to the handle; it may be refilled once clair_wait(slot) has returned. */
int clair_slot_input(clair_engine_t *e, int slot, float **x_pinned);
/* The pipelined call for a producer that holds the RAW pileup counts (dataPrepScripts/CreateTensor.py:29-65: what the text
 * records carry before clair/utils.py:96-98 subtracts channel 0 from channels 1..3): counts [n][33][8][4] int16, half the bytes
 * of the float32 tensor on the host link, which is what bounds the host-buffer boundary.  The subtraction
 * and the conversion run on the device; the results are bit-identical to clair_submit on the float32 tensor utils.py would
 * build from the same counts (every count is exactly representable).  Counts above 32767 do not fit: the caller checks. */
int clair_submit_counts(clair_engine_t *e, int slot, const int16_t *counts, int n, float *gt21, float *genotype,
                        float *indel_len1, float *indel_len2);

/* The pipelined call with the DECODE on the device.  What call_var does with the probabilities of a batch -- the ten outcome families
 * (1 179 float32 products, clair/call_var.py:589-690), the iterative arg-max with exact-equality membership tests (:693-947), genotype,
 * depth, supporting reads and the probability QUAL starts from (:1002-1166) -- runs as one more kernel behind the forward pass, and what
 * comes back per candidate is the 32-byte call record of include/clair_call.h instead of (or besides) the 360 bytes of probabilities.
 * clair_host_format_calls (include/clair_host.h) turns records into VCF rows; clair_host_resolve_calls is the CPU twin of the kernel
 * (bit-identical records).  input: [n][33][8][4] float32 as for clair_submit (input_is_counts == 0) or raw int16 counts as for
 * clair_submit_counts (!= 0); input_stride_bytes = distance between consecutive candidates in the caller's buffer (0 = dense), so that the
 * counts can be taken straight out of an array of binary tensor records (clair_amd/tensor_binary.py: 2 192-byte records) without a
 * host-side copy to make them contiguous.  centre: [n][2] bytes per candidate -- the centre character of its reference window (refseq[16],
 * clair/call_var.py:1015) and min(length of refseq, 255); required when calls != NULL.  calls: caller's array of n records, or NULL.
 * gt21 / genotype / indel_len1 / indel_len2: all four or all NULL (NULL: the probabilities stay on the device).  Pair with
 * clair_wait(slot); buffers must stay valid until it returns.  `input` may also be a DEVICE address of int16 counts (the windows
 * clair_frontend_build_windows leaves in HBM, clair_frontend_counts_device): nothing is copied then. */
int clair_submit_ex(clair_engine_t *e, int slot, const void *input, int input_is_counts, int64_t input_stride_bytes, int n,
                    const uint8_t *centre, clair_call_t *calls, float *gt21, float *genotype, float *indel_len1, float *indel_len2);

/* Page-locked host memory the DMA engine can read in place.  A producer that fills such a buffer -- e.g. reads binary tensor records
 * from a file straight into it -- and passes a pointer INTO it as `input` of clair_submit_ex (with the records' stride) gets the
 * batch to the GPU without any pass over it on the submitting thread: the transfer is a strided 2-D copy from where the data lies.
 * The buffer must not be rewritten before clair_wait of the submit that read it has returned.  Freed by clair_pinned_free (which
 * waits for the handle's streams) or with the engine. */
int clair_pinned_alloc(clair_engine_t *e, int64_t bytes, void **ptr);
int clair_pinned_free(clair_engine_t *e, void *ptr);

/* The decode alone, on probabilities the caller already holds (call_var --input_probabilities, clair/call_var.py:1276-1309, and the
 * tests that feed the kernel crafted probabilities: exact ties, exact zeros, products that underflow).  Synchronous; does not need
 * weights.  x: the candidates' network input [n][33][8][4] float32 (the decode reads depth, supporting reads and the votes on
 * inserted bases from it). */
int clair_decode(clair_engine_t *e, int slot, const float *x, const float *gt21, const float *genotype, const float *indel_len1,
                 const float *indel_len2, int n, const uint8_t *centre, clair_call_t *calls);

/* -- scoring against truth labels on the device: clair.py evaluate (clair/evaluate.py:38-163) ------------------------------------
 * The reference's second consumer of Clair.predict runs the model over a labelled tensor set and accumulates four confusion
 * matrices and the top-1 / top-2 counters of the gt21 head (evaluate.py:87-129).  Here that accumulation is one more kernel behind
 * the forward pass (clair_amd/csrc/evaluate.hip.h), on the slot's own lane like the decode, into a counter block the handle owns in
 * device memory: in evaluation mode only the block ever crosses the host link.  Added without an ABI bump, as the native BAM
 * reader's entry points were; no kernel id (enum clair_kernel_id is what callers size arrays by).
 * Counter block: CLAIR_EVAL_COUNTS int64 = all, top1, top2 (evaluate.py:96-102), then row-major [true][predicted]: gt21 21x21
 * (:92-94), genotype 3x3 (:105-109), indel length 1 33x33 and indel length 2 33x33 (:118-129: the pair of true indices and the pair of
 * predicted arg-maxes are each put in ascending order first).
 * Labels: [n][4] bytes per candidate, the TRUE indices gt21 0..20, genotype 0..2, len1 0..32, len2 0..32 (np.argmax of the four
 * slices of the reference's 90-element label vector, clair/task/main.py:36-81).  A label out of range is an error of the call that
 * takes it, raised on the host before anything is enqueued: the counters stay as they were.
 * Ties: arg-max is the lowest index among equals (np.argmax).  Top-1 / top-2 order: descending probability, then DESCENDING index
 * (a reversed stable sort; the reference's argsort()[::-1], :97, leaves the order among exactly equal values to NumPy's sort).
 * NaN probabilities are out of scope.  The counts are integers added with atomics: they do not depend on launch order or on the
 * number of slots and lanes in flight. */
#define CLAIR_EVAL_COUNTS (3 + 21 * 21 + 3 * 3 + 33 * 33 + 33 * 33) /* 2631 */
/* Allocate the block on first use and zero it (waits for the handle's streams): confusion matrices of evaluate.py:59-64. */
int clair_eval_reset(clair_engine_t *e);
/* m.predict + the scoring of one batch (evaluate.py:81-129), pipelined: input, input_is_counts and input_stride_bytes as for
 * clair_submit_ex (float32 tensor or raw int16 counts, host or device address, strided); forward pass, then the scoring of its
 * probabilities against `labels` ([n][4]; must stay valid until clair_wait, like `input`).
 * gt21 / genotype / indel_len1 / indel_len2: all NULL (the probabilities stay on the device: the normal evaluation mode) or all
 * given (tests).  Pair with clair_wait(slot).  Not available on a handle that opted into the fused layer-2 launch
 * (CLAIR_AMD_LSTM2_FUSED=1): a pass re-run after a misplaced launch would be counted twice. */
int clair_submit_eval(clair_engine_t *e, int slot, const void *input, int input_is_counts, int64_t input_stride_bytes, int n,
                      const uint8_t *labels, float *gt21, float *genotype, float *indel_len1, float *indel_len2);
/* The scoring alone (evaluate.py:87-129), on probabilities the caller holds: synchronous, needs no weights -- the twin of
 * clair_decode, and how crafted rows (exact ties) reach the kernel. */
int clair_eval(clair_engine_t *e, int slot, const float *gt21, const float *genotype, const float *indel_len1, const float *indel_len2,
               const uint8_t *labels, int n);
/* Wait for all slots' device work, then copy the block to counts[CLAIR_EVAL_COUNTS] (what evaluate.py:136-163 prints from). */
int clair_eval_read(clair_engine_t *e, int64_t *counts);

/* -- ensemble calling: K checkpoints over the same candidates, averaged on the device ----------------------------------------------
 * The reference's accuracy lever after training (docs/POST_PROCESSING.md): call_var --output_for_ensemble once per model
 * (clair/call_var.py:950-1000), clair/post_processing/ensemble.py to average the rows of a site (:10-75), call_var
 * --input_probabilities to decode the averages (clair/call_var.py:1276-1309) -- K + 2 processes and 3 KB of text per candidate and
 * model.  Here a handle holds up to CLAIR_ENSEMBLE_MAX_MODELS weight images; one submit brings the batch in once, runs the K forward
 * passes back to back on the slot's lane, folds each into a per-slot accumulator (clair_amd/csrc/ensemble.hip.h) and decodes the
 * averaged rows.  The average is the text chain's, value for value: every probability rounded to six decimals as '{:0.6f}' prints it,
 * re-read as double, summed in model order, divided by K, rounded to six decimals again as '{:.6f}' prints a double (NOT
 * rint(mean * 1e6): docs/ensemble.md), read as float32.  K = 1 therefore is not the identity: it rounds to six decimals, as the chain
 * with one model does.  NaN is out of scope.  Added without an ABI bump and without a kernel id, as clair_eval_* was.
 * Not available on a handle that opted into the fused layer-2 launch (CLAIR_AMD_LSTM2_FUSED=1): a pass re-run after a misplaced
 * launch knows one weight image.  A handle that never calls clair_ensemble_models behaves exactly as before. */
#define CLAIR_ENSEMBLE_MAX_MODELS 8
/* Clair() once per model (clair/model.py:58-192): the handle holds `models` weight images from here on, 1 .. 8.  Image 0 is the one
 * clair_set_tensor / clair_finalize_weights load; images beyond `models` are released.  Waits for the handle's streams. */
int clair_ensemble_models(clair_engine_t *e, int models);
/* Clair.restore_parameters() of model `model` (clair/model.py:1016-1020): as clair_set_tensor / clair_finalize_weights, per image. */
int clair_ensemble_set_tensor(clair_engine_t *e, int model, int tensor_id, const float *host, int64_t count);
int clair_ensemble_finalize_weights(clair_engine_t *e, int model);
/* m.predict of every model + ensemble.py:33-43, :67 + the decode (clair/call_var.py:1331-1352 per model, :1276-1309), pipelined:
 * arguments and input forms exactly those of clair_submit_ex (host or device address, float32 tensor or raw int16 counts, strided;
 * calls and / or the four probability arrays), every image finalized.  The probabilities handed back are the AVERAGED rows, the
 * call records their decode.  Models are summed in image order.  Pair with clair_wait(slot). */
int clair_submit_ensemble(clair_engine_t *e, int slot, const void *input, int input_is_counts, int64_t input_stride_bytes, int n,
                          const uint8_t *centre, clair_call_t *calls, float *gt21, float *genotype, float *indel_len1, float *indel_len2);
/* The averaging alone (ensemble.py:33-43, :67 and the two text conversions around it), on probabilities the caller holds: probs
 * [models][n][90] packed rows (gt21 | genotype | len1 | len2) -> out [n][90].  Synchronous, needs no weights -- the twin of
 * clair_decode / clair_eval, and how crafted rows (exact half-way means) reach the kernel.  clair_host_ensemble_average
 * (include/clair_host.h) is its CPU twin, bit for bit. */
int clair_ensemble_average(clair_engine_t *e, int slot, const float *probs, int models, int n, float *out);

/* -- ensemble across BAMs: sites merged and averaged on the device ------------------------------------------------------------------
 * The reference's post-processing recipe is "many models with many BAMs": the same region called from several (e.g. down-sampled) BAMs
 * with several checkpoints, every run printed with --output_for_ensemble, the rows of a site averaged by
 * clair/post_processing/ensemble.py:10-75.  Different BAMs yield different candidate sites, so beyond the averaging of
 * clair_submit_ensemble this needs a table keyed by position: a SITE TABLE (clair_amd/csrc/sites.hip.h), owned by the engine handle,
 * that holds per site the number of (BAM, model) runs that produced it, the sum of their re-read probabilities in run order (double),
 * and window, centre bytes and reference window of the FIRST run that had it.  Sites are rows in first-seen order -- the order the text
 * chain prints.
 *   for each BAM (a SOURCE):  clair_sites_begin_source with all its candidate positions, strictly ascending, then its batches through
 *                             clair_submit_sites + clair_wait (any slot, any order), every model of the handle over each;
 *   clair_sites_finish:       sites with at least min_count runs (ensemble.py:58-59), in chain or position order, averaged with the
 *                             site's own count as divisor (the rule of csrc/ensemble_core.h);
 *   clair_submit_site_calls:  the decode of a range of the output list, results as from clair_submit_ensemble.
 * A site takes at most CLAIR_SITES_MAX_ROWS runs.  Errors (non-zero, message from clair_last_error of the engine): positions not
 * strictly ascending, a row range outside the current source or the output list, rows after clair_sites_finish, a 65th run of a site
 * (reported by clair_sites_add_rows and clair_sites_finish), a handle with the fused layer-2 launch.  clair_host_sites_*
 * (include/clair_host.h) is the CPU twin, bit for bit.  Added without an ABI bump, as clair_ensemble_* was. */
#define CLAIR_SITES_MAX_BAMS 8
#define CLAIR_SITES_MAX_ROWS 64 /* CLAIR_SITES_MAX_BAMS * CLAIR_ENSEMBLE_MAX_MODELS */
#define CLAIR_SITES_ORDER_CHAIN 0    /* first-seen order over "for each BAM, for each model": what `cat runs | ensemble` prints */
#define CLAIR_SITES_ORDER_POSITION 1 /* the same rows sorted by position */
typedef struct clair_sites clair_sites_t;
/* A table of the engine; what is not destroyed goes with the engine (destroy tables BEFORE clair_engine_destroy, or not at all). */
int clair_sites_create(clair_engine_t *e, clair_sites_t **out);
void clair_sites_destroy(clair_sites_t *t);
/* Begin the next source: positions [n] strictly ascending (n = 0: an empty source).  Waits for every slot, looks the positions up,
 * gives those not yet in the table rows n_sites .. in ascending order, and leaves the row of every position on the device for the
 * source's batches.  *n_new (optional): how many were new. */
int clair_sites_begin_source(clair_sites_t *t, const int64_t *positions, int64_t n, int64_t *n_new);
/* Candidates [first, first + n) of the current source: input, input_is_counts, input_stride_bytes exactly as for clair_submit_ex
 * (float32 tensor or raw int16 counts, host or device address, strided); centre [n][2] as there, seq [n][33] the reference windows
 * (NUL-padded).  Every weight image of the handle runs over the batch (one without clair_ensemble_models); each pass is added to the
 * sites' sums and counts, and sites nobody wrote before take window, centre and seq of this batch.  Nothing comes back: pair with
 * clair_wait(slot); the buffers must stay valid until it returns. */
int clair_submit_sites(clair_engine_t *e, int slot, clair_sites_t *t, int64_t first, const void *input, int input_is_counts,
                       int64_t input_stride_bytes, int n, const uint8_t *centre, const uint8_t *seq);
/* One run's rows alone, on probabilities the caller holds: probs [n][90] packed rows for candidates [first, first + n) of the current
 * source; x [n][33][8][4] float32, centre [n][2], seq [n][33]: each optional, what new sites take along (zeros for what is not given).  Synchronous, slot 0's
 * buffers, needs no weights -- the twin of clair_ensemble_average, and how crafted rows reach the table. */
int clair_sites_add_rows(clair_engine_t *e, clair_sites_t *t, int64_t first, const float *probs, int n, const float *x,
                         const uint8_t *centre, const uint8_t *seq);
/* Close the table and make its output list; may be repeated with another min_count or order.  *n_out: sites in the list. */
int clair_sites_finish(clair_sites_t *t, int min_count, int order, int64_t *n_out);
/* Entries [first, first + n) of the output list: positions [n], counts [n], seq [n][33] (each optional); the averaged rows [n][90];
 * the windows [n][33][8][4] float32. */
int clair_sites_info(clair_sites_t *t, int64_t first, int64_t n, int64_t *positions, int32_t *counts, uint8_t *seq);
int clair_sites_rows(clair_sites_t *t, int64_t first, int64_t n, float *out);
int clair_sites_windows(clair_sites_t *t, int64_t first, int64_t n, float *x);
/* Decode entries [first, first + n) of the output list on slot `slot`: call records and / or the averaged probabilities, exactly as
 * clair_submit_ensemble hands them back.  Needs no weights.  Pair with clair_wait(slot). */
int clair_submit_site_calls(clair_engine_t *e, int slot, clair_sites_t *t, int64_t first, int n, clair_call_t *calls, float *gt21,
                            float *genotype, float *indel_len1, float *indel_len2);

/* -- device-resident candidate sets (benchmark / multi-GPU shard driver) ------------------------
 * The candidate set lives in HBM: x_dev [N,33,8,4]; outputs out_dev [N,90] rows laid out
 * gt21(21) | genotype(3) | len1(33) | len2(33).  clair_run_resident enqueues the forward pass
 * for candidates [first, first+n) on slot `slot` (no host copies) and returns immediately;
 * clair_sync waits for all slots. */
int clair_dataset_alloc(clair_engine_t *e, int64_t n_candidates, void **x_dev, void **out_dev);
int clair_dataset_free(clair_engine_t *e, void *x_dev, void *out_dev);
int clair_dataset_upload(clair_engine_t *e, void *x_dev, int64_t first, const float *x_host, int64_t n);
int clair_dataset_download(clair_engine_t *e, const void *out_dev, int64_t first, float *out_host, int64_t n);
int clair_run_resident(clair_engine_t *e, int slot, const void *x_dev, void *out_dev, int64_t first, int n);
int clair_sync(clair_engine_t *e);

/* -- measurement ---------------------------------------------------------------------------------
 * When enabled, every kernel launch is bracketed by HIP events on the slot's own stream.
 * clair_kernel_times returns, per kernel id, the summed duration in milliseconds and the number
 * of launches since the last reset (it synchronises first).
 * on: 0 = off, 1 = every kernel, any other value = bit mask over enum clair_kernel_id (bit k = kernel k; bit 0 names an
 * unused id, so 1 is unambiguous): a pass that times ONE kernel adds two marker packets per forward pass instead of ten. */
int clair_timing_enable(clair_engine_t *e, int on);
int clair_kernel_times(clair_engine_t *e, double *ms_sum /*[CLAIR_K_COUNT]*/, int64_t *launches /*[CLAIR_K_COUNT]*/);
int clair_timing_reset(clair_engine_t *e);
/* Launch geometry: the number of 256-thread workgroups each kernel id is launched with for a batch of n candidates on this
 * handle (0 for ids that launch nothing).  The recurrent kernels and, on handles with several slots, the projection GEMM are
 * sized to PART of the chip so that the batches in flight on other slots run beside them; a per-kernel roofline needs that share. */
int clair_kernel_workgroups(clair_engine_t *e, int n, int *workgroups /*[CLAIR_K_COUNT]*/);

/* Event counters of the handle.  which: 0 = forward passes launched with the fused layer-2 kernel (one launch for the LSTM2
 * projection and recurrence, used on handles with one or two slots), 1 = forward passes that were RE-RUN on the two-launch path
 * because a fused launch reported that its workgroups were not placed as it assumes.  A re-run is invisible to the caller
 * (same arithmetic, same outputs; the reference never drops a batch, clair/call_var.py:1331-1352) except through this counter
 * and one line on stderr; after the first one the handle stays on the two-launch path. */
int clair_engine_counter(clair_engine_t *e, int which, int64_t *value);

/* -- layer taps for parity tests: copy an intermediate of the LAST forward pass run on `slot`
 *    to the host.  which: 1 = LSTM1 output [33,n_pad,256], 2 = LSTM2 output [33,n_pad,256],
 *    3 = split-K partials of the L4 product [8,n_pad,192], 4 = L3 output [n_pad,7680] (only when the engine was created
 *    with CLAIR_AMD_TAP_L3=1 in the environment)
 *    (L3/L4 activations only ever exist in LDS / split-K partials).  n_pad = n rounded up to 32. */
int clair_debug_read(clair_engine_t *e, int slot, int which, float *host, int64_t count);

/* -- multi-GPU: one process per GPU, candidates shard in contiguous blocks of whole batches -------------------------------
 * The reference scales out by running one callVarBam per 10 Mbp chunk under GNU parallel and concatenating the chunk VCFs
 * (clair/callVarBamParallel.py:90-119, README.md:297-303); candidates are classified independently
 * (docs/POST_PROCESSING.md:17).  Here rank r owns a contiguous block of the candidate stream (clair_amd/shard.py) and the
 * forward pass needs NO collective.  This communicator is a thin binding of RCCL (xGMI between the GPUs of a node) for
 * the trivial parts only: the weight blob from rank 0 (9.5 MB, once), the gather of per-rank output rows, counters and timers.
 * librccl.so is loaded on the first call.  Rendezvous: rank 0 calls clair_comm_unique_id and hands the 128 bytes to the
 * other ranks out of band (clair_amd/shard.py uses a socket on 127.0.0.1); every rank then calls clair_comm_create
 * (collective: returns once all `world` ranks have joined).  All calls are blocking; host buffers are staged through HBM. */
#define CLAIR_COMM_ID_BYTES 128
enum clair_comm_op { CLAIR_COMM_SUM = 0, CLAIR_COMM_MAX = 1, CLAIR_COMM_MIN = 2 };
typedef struct clair_comm clair_comm_t;
/* Everything clair_comm_create needs that can be checked WITHOUT the other ranks: a HIP device with this ordinal that accepts an
 * allocation, librccl.so loadable with the entry points bound.  The ranks exchange the result out of band before any of them
 * enters the collective ncclCommInitRank, so one rank's failure is an error on every rank instead of a hang on the others. */
int clair_comm_preflight(int device);
int clair_comm_unique_id(uint8_t *id /*[CLAIR_COMM_ID_BYTES]*/);                 /* ncclGetUniqueId */
int clair_comm_create(int device, int rank, int world, const uint8_t *id, clair_comm_t **out);   /* ncclCommInitRank */
void clair_comm_destroy(clair_comm_t *c);
/* Tear-down that does not wait for the peers (ncclCommAbort): for a communicator that came up on this rank while a peer's
 * clair_comm_create failed, and for the helper thread of clair_comm_create_timed when RCCL returns after its deadline. */
void clair_comm_abort(clair_comm_t *c);
/* clair_comm_create with a deadline (round 6; ABI 6): ncclCommInitRank AND the first collective on the new communicator (one
 * all-reduce: RCCL connects its transports lazily) run on a helper thread; 0 = up and proven, 1 = failed (clair_comm_last_error(NULL)),
 * CLAIR_COMM_TIMED_OUT = neither returned within `timeout_ms`.  On a time-out no communicator exists for the caller: the helper thread
 * is abandoned and aborts its communicator should RCCL ever return (until then a thread of this process sits inside librccl: leave the
 * process with _exit once the results are written -- exit() would run librccl's static destructors under it).  clair_amd/shard.py then tells the peers over the bootstrap
 * sockets and every rank goes on over the socket transport -- a hung RCCL bring-up still yields the N-rank line (`rccl_failure`). */
#define CLAIR_COMM_TIMED_OUT 2
int clair_comm_create_timed(int device, int rank, int world, const uint8_t *id, int timeout_ms, clair_comm_t **out);
const char *clair_comm_last_error(const clair_comm_t *c);                         /* c may be NULL: failure of create / unique_id */
int clair_comm_barrier(clair_comm_t *c);
int clair_comm_allreduce_f64(clair_comm_t *c, double *values /*in place*/, int count, int op /*enum clair_comm_op*/);
int clair_comm_broadcast(clair_comm_t *c, void *host, int64_t bytes, int root);  /* ncclBroadcast of a host buffer (the weight blob) */
int clair_comm_allgather(clair_comm_t *c, const void *send_host, void *recv_host /*[world][bytes_per_rank]*/, int64_t bytes_per_rank);
/* the same on HBM-resident buffers (e.g. the out_dev rows of clair_dataset_alloc), no host staging */
int clair_comm_allgather_device(clair_comm_t *c, const void *send_dev, void *recv_dev, int64_t bytes_per_rank);

/* ---- front end on the device: alignments -> candidate sites -> pileup windows that stay in HBM -----------------------------------
 *
 * Stands behind the two pypy stages callVarBam pipes into call_var (clair/callVarBam.py:124-199):
 *   dataPrepScripts/ExtractVariantCandidates.py:160-393 (make_candidates)   -> clair_frontend_find_candidates
 *   dataPrepScripts/CreateTensor.py:173-388 (OutputAlnTensor), :29-65       -> clair_frontend_build_windows
 *   clair/utils.py:90-98 (centre-base filter; the channel subtraction is clair_submit_ex's, input_is_counts)
 * Input: slabs of packed alignments (include/clair_reads.h, produced from `samtools view` text by clair_host_sampack_*), the
 * reference bases both stages index (`samtools faidx` of the region widened by 1 Mbp, upper-cased; reference_start_0_based = 0-based
 * position of its first base), and the span of 0-based reference positions [span_lo, span_hi) the per-position tables cover
 * (alignment bases outside it are ignored: make it the region plus a margin of >= 64).  Output: n windows of [33][8][4] int16 counts
 * in device memory (clair_frontend_counts_device -> clair_submit_ex with input_is_counts = 1), their centres (1-based) and the 33
 * reference bases under them.  Windows are the ones the sequential stages write, in ascending order, bit for bit, PROVIDED no
 * CLAIR_FE_* bit (clair_reads.h) is set in stats[0] and the tuple budget did not bind (clair_frontend_budget_inputs ->
 * clair_host_tuple_budget_binds); otherwise the caller runs clair_host_evc_* / clair_host_pileup_*, which reproduce the reference
 * in every regime.
 * Calls on one handle are not concurrent; all are synchronous. */
typedef struct clair_frontend clair_frontend_t;
struct clair_read;
struct clair_op;
int clair_frontend_create(int device, const char *ref_seq, int64_t ref_len, int64_t reference_start_0_based, int64_t span_lo, int64_t span_hi,
                          clair_frontend_t **out);
void clair_frontend_destroy(clair_frontend_t *f);
const char *clair_frontend_last_error(const clair_frontend_t *f);      /* f may be NULL: failure of create */
/* Copy one slab to the device (it stays there) and add its bases to the per-position tables.  The arrays may be reused on return.
 * The alignments of a slab are expected in ascending order of pos0 (what `samtools view` of a sorted BAM prints and both packers
 * keep); a slab whose starts decrease is still tallied correctly (by the order-independent per-base kernel) and sets
 * CLAIR_FE_UNSORTED in stats[0] of clair_frontend_stats, like the packers do: the reference's scripts would have stopped there. */
int clair_frontend_add_reads(clair_frontend_t *f, const struct clair_read *reads, int64_t n_reads, const struct clair_op *ops, int64_t n_ops,
                             const uint32_t *op_elem, const uint8_t *seq, int64_t seq_bytes);
/* ... or hand over the `samtools view` TEXT and let the device do the packing as well: the line handling of both scripts
 * (ExtractVariantCandidates.py:266-295, CreateTensor.py:251-287) one thread per line, exactly what clair_host_sampack_* produces
 * (arguments of _text_options as clair_host_sampack_create); of the text only the SEQ columns of the kept alignments stay on the device.  `sam` holds whole
 * lines (the caller keeps an unfinished last line for the next call), at most 2 GB at a time; the --dcov and sortedness state runs on
 * across calls.  Returns 2 when a line is malformed (too few columns, a non-integer FLAG / POS / MAPQ): clair_host_sampack_feed on
 * the same text reports it the way the host path does.  _text_stats: stats[0..3] = lines, candidate-search alignments, pileup
 * alignments since _text_options, CLAIR_FE_* bits of the line handling (also folded into clair_frontend_stats).  _slab_reads copies
 * a slab's alignment records back (the budget replay walks them); reads == NULL only asks for the count. */
int clair_frontend_text_options(clair_frontend_t *f, const char *ctg_name, int dcov, int evc_min_mq, int pile_min_mq, int64_t pile_start, int64_t pile_end);
int clair_frontend_add_text(clair_frontend_t *f, const char *sam, int64_t len);
int clair_frontend_text_stats(clair_frontend_t *f, int64_t *stats);
int clair_frontend_slab_reads(clair_frontend_t *f, int64_t slab, struct clair_read *reads, int64_t capacity, int64_t *n_reads);
/* The binary twins of _text_options / _add_text (callVarBam --bam_reader native): BAM records as the host inflated them (include/clair_host.h:
 * clair_host_bam_next), offsets[k] = where record k starts in records[0 .. len).  The device decodes each record and applies what
 * `samtools view -F 2316 <bam> <region>` applies -- FLAG & 2316 == 0, reference id == tid, overlap (bam_endpos) with region_lo .. region_hi
 * (1-based inclusive; -1 -1 = the whole contig) -- then handles the lines that view prints exactly as _add_text handles the same lines of
 * text (the placeholder CIGAR of a record with more than 65 535 operations replaced by its CG tag, SEQ '*' for l_seq 0): same
 * _text_stats, same slabs.  The other arguments as _text_options.  _add_bam returns 2 when a record's sizes do not fit its block_size
 * (the message names the record's index in the chunk). */
int clair_frontend_bam_options(clair_frontend_t *f, int tid, int dcov, int evc_min_mq, int pile_min_mq, int64_t pile_start, int64_t pile_end,
                               int64_t region_lo, int64_t region_hi);
int clair_frontend_add_bam(clair_frontend_t *f, const uint8_t *records, int64_t len, const int64_t *offsets, int64_t n_records);
/* After _bam_options, before the first _add_bam: keep != 0 packs for the indel look-up (include/clair_reads.h, "the indel look-up") -- every
 * record the view prints that has a CIGAR gets CLAIR_READ_LOOKUP and stays in the slab even when neither stage walks it (low MQ, beyond
 * --dcov: pysam's pileup, which clair/call_var.py:102-170 reads, applies neither).  A sibling of _bam_options because that call's argument
 * list is fixed.  Off: slabs as ever, byte for byte; on: the same candidates and windows (the stages skip what carries neither EVC nor PILE). */
int clair_frontend_bam_lookup(clair_frontend_t *f, int keep);
/* After _bam_options, before the first _add_bam (afterwards an error, as _bam_lookup's): one more clause of the view, what `samtools view -s`
 * adds to it -- a record the rest of the view prints is dropped when the hash of its read name, XORed with the 32-bit word `seed`
 * (0 .. 2^32 - 1) and mixed, falls at or above `frac` (csrc/subsample_core.h, docs/subsample.md; the host twin is
 * clair_host_bam_set_subsample).  frac <= 0 turns the rule off, frac >= 1 keeps every record.  It runs in the thread that decodes the
 * record, before --dcov, _text_stats and everything downstream, which see fewer lines; a malformed record is reported whether or not the
 * rule would have dropped it.  _bam_options resets it to off. */
int clair_frontend_bam_subsample(clair_frontend_t *f, int64_t seed, double frac);
/* insertion_bases_using_pysam_from / deletion_bases_using_pysam_from (clair/call_var.py:102-170; asked for at :498-565 and :805-823) for n
 * positions in ONE call, from the slabs resident on the device (csrc/indel_lookup.hip: one thread per I / D operation finds its query,
 * one wave per query groups its hits by key).  positions[n]: 1-based, strictly ascending.  entries: [n][capacity] (capacity 1 .. 65536),
 * n_entries[n], depth[n], status[n] (CLAIR_LOOKUP_*): the table defined in include/clair_reads.h, byte for byte what
 * clair_host_indel_table (include/clair_host.h) writes for the same slabs -- a query the device cannot finish (CLAIR_LOOKUP_HITS) is
 * answered by that code over the slabs copied back.  Works before and after the candidates are fixed.  Synchronous. */
struct clair_indel_entry;
int clair_frontend_indel_table(clair_frontend_t *f, const int64_t *positions, int64_t n, struct clair_indel_entry *entries, int capacity,
                               int32_t *n_entries, int32_t *depth, uint32_t *status);
/* The candidate filter over the tallies: arguments as clair_host_evc_create (include/clair_host.h). */
int clair_frontend_find_candidates(clair_frontend_t *f, double min_coverage, double threshold, int64_t ctg_start, int64_t ctg_end,
                                   const int64_t *bed_start, const int64_t *bed_end, int64_t n_bed, int64_t *n_candidates);
/* ... or a given list (--vcf_fn; 1-based, strictly ascending, else CLAIR_FE_CANDIDATES); positions outside the span are dropped. */
int clair_frontend_set_candidates(clair_frontend_t *f, const int64_t *positions, int64_t n_positions, int64_t *n_candidates);
int clair_frontend_get_candidates(clair_frontend_t *f, int64_t *positions /*[n_candidates]*/);
/* Second pass over the resident alignments + assembly.  min_coverage: CreateTensor's --minCoverage (depth at the centre);
 * drop_non_iupac_centre != 0 applies clair/utils.py:90-91 as well. */
int clair_frontend_build_windows(clair_frontend_t *f, int min_coverage, int drop_non_iupac_centre, int64_t *n_windows);
/* The same with CreateTensor's --stop_consider_left_edge (consider_left_edge = 0, CreateTensor.py:103-104): a read opens a window only
 * by walking its first column, so a read that starts inside a window adds nothing to it; the per-position tables hold such reads too
 * and what they added is collected per window and taken out again. */
int clair_frontend_build_windows_ex(clair_frontend_t *f, int min_coverage, int drop_non_iupac_centre, int consider_left_edge, int64_t *n_windows);
int clair_frontend_window_info(clair_frontend_t *f, int64_t first, int64_t n, int64_t *centres, char *refseq /*[n][34], NUL-padded*/);
int clair_frontend_window_counts(clair_frontend_t *f, int64_t first, int64_t n, int16_t *counts /*[n][33][8][4], host*/);
const int16_t *clair_frontend_counts_device(clair_frontend_t *f, int64_t first);   /* device address of window `first`; NULL before build_windows */
/* -- the training set (python -m clair_amd.make_train_set; csrc/train_set.hip, the rules in csrc/train_set_core.h, docs/train_set.md).
 * _sample_candidates takes the place of _find_candidates: the eligible positions are those of its rule with threshold 0 (what
 * ExtractVariantCandidates.py --gen4Training makes of it); one that is no truth position stays when its draw u(key, position) <=
 * p_near (its nearest truth position is 15 or 16 away) or p_outside (every other one).  truth_positions [n_truth]: 1-based, ascending,
 * duplicates allowed.  add_truth != 0 adds the truth positions inside [ctg_start, ctg_end] to the list.  n_near / n_outside: the
 * sampled sites per class, the reference's two log counters.  key: clair_host_train_set_key(ctg, seed, 1) (include/clair_host.h).
 * _pair, after _build_windows: PairWithNonVariants.py over those windows -- v windows at a truth position, c usable non-variant
 * windows (position, as it stands, inside the bed; n_bed < 0: no bed file), r = min(1, v amp / c), kept: the v windows, then the usable
 * ones with u(key, position) < r (key of stage 2), each part in position order -- and get_training_array's labels: truth_labels
 * [n_truth][4] true indices per truth row (the last row of a position wins), homozygous reference of the centre base elsewhere; a row
 * is in the data set when its position is inside the bed and its centre base is one of ACGTU.
 * stats[5] = v, c, kept variant windows, kept non-variant windows, rows in the data set.
 * _train_set_info / _train_set_counts: rows [first, first + n) of the kept list, the counts gathered on the device.
 * clair_host_train_set_* (include/clair_host.h) gives the same bytes on the CPU. */
int clair_frontend_sample_candidates(clair_frontend_t *f, double min_coverage, int64_t ctg_start, int64_t ctg_end, const int64_t *bed_start, const int64_t *bed_end,
                                     int64_t n_bed, const int64_t *truth_positions, int64_t n_truth, double p_near, double p_outside, int64_t key, int add_truth,
                                     int64_t *n_candidates, int64_t *n_near, int64_t *n_outside);
int clair_frontend_pair(clair_frontend_t *f, const int64_t *truth_positions, const uint8_t *truth_labels, int64_t n_truth, const int64_t *bed_start,
                        const int64_t *bed_end, int64_t n_bed, double amp, int64_t key, int64_t *stats);
int clair_frontend_train_set_info(clair_frontend_t *f, int64_t first, int64_t n, int64_t *centres, char *refseq, uint8_t *labels, uint8_t *in_set);
int clair_frontend_train_set_counts(clair_frontend_t *f, int64_t first, int64_t n, int16_t *counts);
/* What the budget replay needs: tuples appended per alignment of slab `slab` (read_tuples, may be NULL), all candidate centres and
 * the tuples each window held (0 for a window no alignment opened); either pair may be NULL. */
int clair_frontend_budget_inputs(clair_frontend_t *f, int64_t slab, uint64_t *read_tuples, int64_t *centres, uint64_t *window_tuples);
/* stats[0..5] = CLAIR_FE_* bits seen on the device, slabs, alignments, elements, candidates (-1: not yet), windows (-1: not yet) */
int clair_frontend_stats(clair_frontend_t *f, int64_t *stats);

/* -- gVCF: reference-confidence blocks from the candidate search's tallies (csrc/gvcf.hip, rule in csrc/gvcf_core.h; docs/gvcf.md).
 *    Stands for nothing in the reference, which writes no gVCF: the yardstick is the restatement in tests/gvcf_cases.py, the format is
 *    GATK's (blocks written 0/0 with END, GQ, DP, MIN_DP, PL and banded by GQ).
 *    _position_tallies: the seven tallies A C G T I D N of 0-based positions [first, first + n), which lie inside the tables, into out
 *      [n][7] -- the numbers fe_candidate_flags_kernel tests (ExtractVariantCandidates.py:296-316), so that a wrong count can be told
 *      from a wrong rule.
 *    _gvcf_blocks: the costs c_match, c_err, c_half (1/1024 phred, each 1 .. 2^17 - 1), band_of_gq [100] (the band index of GQ 0 .. 99,
 *      not decreasing) and the allowed set as n_iv sorted, disjoint, 0-based half-open intervals inside the tables.  *n_blocks = the
 *      number of blocks; when capacity >= that number the records are copied to out (a second call with the same arguments only
 *      copies).  Returns 2 with a verdict in clair_frontend_last_error for a bad argument (the handle stays usable; the host twin
 *      clair_host_gvcf_blocks words it the same way), 3 when the front end reported a CLAIR_FE_* bit: its tallies may be incomplete,
 *      the caller runs the host twin.
 *    _gvcf_device_ms: milliseconds between two events around the launches of the last computation (class kernel, scan, record writer;
 *      the host reads the block count in between), for docs/gvcf.md's numbers. */
#ifndef CLAIR_GVCF_TYPES
#define CLAIR_GVCF_TYPES
typedef struct clair_gvcf_block {
    int64_t start, end;      /* 0-based, half-open */
    uint32_t min_dp, dp;     /* the smallest DP of the block; floor(sum of DP / length) */
    int32_t gq;              /* the smallest GQ of the block */
    int32_t pl[3];           /* per genotype 0/0, 0/1, 1/1 the smallest PL of the block */
} clair_gvcf_block_t;        /* 40 bytes */
#endif
int clair_frontend_position_tallies(clair_frontend_t *f, int64_t first, int64_t n, uint32_t *out);
int clair_frontend_gvcf_blocks(clair_frontend_t *f, int c_match, int c_err, int c_half, const uint8_t *band_of_gq, const int64_t *iv_start, const int64_t *iv_end,
                               int64_t n_iv, clair_gvcf_block_t *out, int64_t capacity, int64_t *n_blocks);
int clair_frontend_gvcf_device_ms(clair_frontend_t *f, double *ms);

/* -- BGZF inflate on the device (callVarBam --bam_inflate device; csrc/inflate.hip, docs/bam_reader.md).  A handle owns one stream and
 * page-locked staging plus device buffers for max_blocks blocks (64 KiB each, both directions), reused by every call.
 * _blocks: n <= max_blocks whole BGZF blocks (header and footer included) at cdata[in_at[i] .. + csize[i]), csize >= 26; block i's
 * inflated bytes go to out[out_at[i] .. + out_len[i]) where out_len is the block's ISIZE (<= 65536) and every output range lies in
 * [0, max_blocks * 65536).  status[i]: 0 ok, 1 corrupt deflate data, 2 inflated size differs from ISIZE, 3 CRC32 mismatch; the
 * output range of a block whose status is not 0 is left untouched, and no block disturbs another.  Synchronous.  Returns 0 when the
 * batch ran, whatever the statuses; non-zero for a bad argument (nothing is enqueued then) or a HIP error.
 * _blocks_cb is the same function in the shape clair_host_bam_set_inflater takes (include/clair_host.h), the handle as its context. */
typedef struct clair_inflate clair_inflate_t;
int clair_inflate_create(int device, int max_blocks, clair_inflate_t **out);
void clair_inflate_destroy(clair_inflate_t *h);
const char *clair_inflate_last_error(const clair_inflate_t *h);        /* h may be NULL: failure of create */
int clair_inflate_blocks(clair_inflate_t *h, const uint8_t *cdata, int64_t cbytes, int n, const int64_t *in_at, const int32_t *csize,
                         const int64_t *out_at, const int32_t *out_len, uint8_t *out, int32_t *status);
int clair_inflate_blocks_cb(void *handle, const uint8_t *cdata, int64_t cbytes, int n, const int64_t *in_at, const int32_t *csize,
                            const int64_t *out_at, const int32_t *out_len, uint8_t *out, int32_t *status);

/* -- BGZF deflate on the device (merge_vcf --bgzf_deflate device; csrc/deflate.hip, docs/merge_vcf.md).  The writer's side of the above: a
 * handle owns one stream, page-locked staging and device buffers for max_blocks (1 .. 16384) blocks, reused by every call.
 * _blocks: n <= max_blocks payloads data[in_at[i] .. + in_len[i]), 0 <= in_len <= 65280, every range inside data[0 .. bytes) -> block i as
 * one whole BGZF block (18-byte header with BSIZE, raw deflate stream, CRC-32, ISIZE) in out[i * 65536 .. + csize[i]); the rest of its
 * 65536-byte slot is zeroed.  A wave per block; the bytes are those clair_host_deflate_bgzf (include/clair_host.h) gives for the same
 * payload.  Synchronous.  Returns non-zero for a bad argument (nothing is enqueued then) or a HIP error. */
typedef struct clair_deflate clair_deflate_t;
int clair_deflate_create(int device, int max_blocks, clair_deflate_t **out);
void clair_deflate_destroy(clair_deflate_t *h);
const char *clair_deflate_last_error(const clair_deflate_t *h);        /* h may be NULL: failure of create */
int clair_deflate_blocks(clair_deflate_t *h, const uint8_t *data, int64_t bytes, int n, const int64_t *in_at, const int32_t *in_len,
                         uint8_t *out, int32_t *csize);

/* -- the overlap filter on the device (call_var / callVarBam --overlap_filter device; csrc/overlap.hip, docs/overlap_variant.md).
 * The walk of clair/post_processing/overlap_variant.py:237-267 over n rows reduced to 24-byte spans (csrc/overlap_core.h lays the
 * record out and holds the pair rule): spans [n] in input order, host memory -> keep [n], host memory, 1 for every row the filter
 * prints.  Exact for every input, unsorted ones included: rows no earlier row of their contig run can overlap are found with a
 * segmented max-scan, and one lane walks each stretch between two of them with the sequential rule.  Synchronous; the device memory
 * lives for the call.  Returns non-zero for a bad argument, a missing device or a HIP error, with a message in _last_error (one per
 * process).  clair_host_overlap_keep (include/clair_host.h) gives the same bytes on the CPU. */
#ifndef CLAIR_OVERLAP_SPAN_T
#define CLAIR_OVERLAP_SPAN_T
typedef struct clair_overlap_span clair_overlap_span_t;
#endif
int clair_overlap_keep(int device, const clair_overlap_span_t *spans, int64_t n, uint8_t *keep);
const char *clair_overlap_last_error(void);

/* -- training on the device (python -m clair_amd.train, Clair.train / validate; csrc/train.hip, docs/train.md).
 * A trainer is its own handle and needs no engine: float32 copies of the 22 tensors of enum clair_tensor_id in four sets (0 weights,
 * 1 gradients, 2 Adam m | momentum accumulator, 3 Adam v), and the workspace of one micro-batch of at most `micro_batch` rows (the gates,
 * cell states and dropout masks of both LSTM layers over 33 steps: about 0.59 MB a row).  optimizer: 0 Adam, 1 momentum SGD (0.9, no
 * Nesterov).  loss: 0 focal loss (clair/model.py:784-805), 1 weighted cross entropy (:247-263).  Every call is synchronous.
 * _set_tensor / _get_tensor: one tensor of one set, `count` floats, shapes as enum clair_tensor_id.
 * _config: task_loss_weights [5] (gt21, genotype, len1, len2, l2), class_weights [90] (cross entropy; packed as the outputs are),
 *   dropout_rates [6] (LSTM2, L4, L5_1..4) -- a NULL array keeps what the handle has -- and the seed of the dropout masks.
 * _accumulate: one micro-batch, x [n,33,8,4] and labels [n,4] true indices, n <= micro_batch; first_row is the position of its first row
 *   in the whole batch (a dropout mask is a hash of seed, optimizer step, layer, row of the whole batch and element, so it does not
 *   depend on how the batch is cut).  training = 0: the forward pass without dropout and the loss (validate).  training = 1: dropout,
 *   and the backward pass ADDS into the gradient set.  losses [4]: the heads' losses summed over the rows, without task weights.
 * _step: adds task_loss_weights[4] * l2_lambda * w to the gradients of the 11 kernels, clips by the global norm of all 22 at 5.0 and applies
 *   the optimizer as TensorFlow 1.x does; stats [2]: sum w^2 / 2 over the kernels before the update, the global norm before clipping.
 *   The gradient set is left holding the regularised, unclipped gradients; _zero_grad clears it.
 * _read_mask: the mask bytes of the last training accumulate, layer 0 LSTM2 [33][n][256], 1 L4 [n][192], 2..5 L5_1..4 [n][96].
 * _probabilities: the packed rows [n,90] of the last accumulate.
 * _accuracy: tp [4], how many rows of the last accumulate (either mode) each head gets right under the learning-rate finder's rule
 *   (clair/learning_rate_finder.py:21-73), counted on the device from the probabilities and labels where they lie (csrc/train_accuracy.hip.h):
 *   tp[0] arg-max of the 21 gt21 probabilities = label, tp[1] the same for the genotype; the indel lengths as sorted pairs -- tp[2] the smaller
 *   of the two arg-maxes = the smaller of the two labels, tp[3] the larger = the larger.  Arg-max is the lowest index among equal values.
 * Non-zero on failure, message from clair_train_last_error (NULL handle: the failure of create). */
typedef struct clair_trainer clair_trainer_t;
int clair_train_create(int device, int micro_batch, int optimizer, int loss, clair_trainer_t **out);
void clair_train_destroy(clair_trainer_t *t);
const char *clair_train_last_error(const clair_trainer_t *t);
int clair_train_set_tensor(clair_trainer_t *t, int set, int tensor_id, const float *host, int64_t count);
int clair_train_get_tensor(clair_trainer_t *t, int set, int tensor_id, float *host, int64_t count);
int clair_train_config(clair_trainer_t *t, const double *task_loss_weights, const double *class_weights, const double *dropout_rates, int64_t seed);
int clair_train_zero_grad(clair_trainer_t *t);
int clair_train_accumulate(clair_trainer_t *t, const float *x, const uint8_t *labels, int n, int64_t first_row, int training, double *losses);
int clair_train_step(clair_trainer_t *t, double learning_rate, double l2_lambda, double *stats);
int clair_train_read_mask(clair_trainer_t *t, int layer, uint8_t *host, int64_t count);
int clair_train_probabilities(clair_trainer_t *t, float *out);
int clair_train_accuracy(clair_trainer_t *t, int64_t *tp);
/* -- kernel taps for tests (tests/test_train_kernels_gpu.py; docs/train.md): one launch of tgemm (csrc/train_gemm.hip.h) or of
 *    column_sum_kernel (csrc/train_kernels.hip.h) on host arrays, through the launch code the trainer itself uses and on its stream.  The
 *    arrays are copied to buffers the handle owns -- C and out go up as well, since `accumulate` and the column sums' += read them and
 *    elements the kernel does not address must come back as they went -- and C / out are copied back.  Synchronous.
 * _debug_gemm: C[b] (+)= A[b] . B[b] (+ bias[b][col]) with A(m, k) = a[b * ba + m * sam + k * sak], B(k, n) = b[b * bb + k * sbk + n * sbn],
 *   C(m, n) = c[b * bc + m * scm + n * scn], bias column n = bias[b * bbias + n].  dims [5] = M, N, K, batch, accumulate (0 | 1);
 *   strides [10] = sam, sak, sbk, sbn, scm, scn, ba, bb, bc, bbias, in elements.  bias NULL with bias_count 0: no bias.
 * _debug_column_sum: out[(j / d) * s1 + (j % d) * s2] += sum over r < rows of x[r * ld + j], j < cols.
 * Nothing is launched unless every address is inside its array: M, N, K, cols 1 .. 2^20, batch 1 .. 65535, rows 1 .. 2^28, every count
 *   1 .. 2^28, every stride, batch offset and ld 0 .. 2^28, d 1 .. 2^28, and the largest element index of each operand -- for A
 *   (M-1)*sam + (K-1)*sak + (batch-1)*ba, and so on -- below its count; otherwise non-zero and a message that names the operand. */
int clair_train_debug_gemm(clair_trainer_t *t, const float *a, int64_t a_count, const float *b, int64_t b_count, const float *bias, int64_t bias_count,
                           float *c, int64_t c_count, const int64_t *dims, const int64_t *strides);
int clair_train_debug_column_sum(clair_trainer_t *t, const float *x, int64_t x_count, int64_t rows, int cols, int64_t ld, float *out, int64_t out_count,
                                 int d, int s1, int s2);

/* -- compare_vcf on the device (python -m clair_amd.compare_vcf --backend device; csrc/compare.hip, docs/compare_vcf.md has the rule and
 * the tables).  One handle scores one call set against one truth set: both texts (VCF as plain bytes, each below 2^32 bytes) are copied to
 * the device, parsed there into 32-byte allele records that point into them (csrc/compare_core.h lays the record out and holds the rule),
 * joined and counted; only statistics, the counter block and, when asked for, the records cross the host link.  side: 0 calls, 1 truth.
 * _set_contigs: the contig table, name k = names[offsets[k] .. offsets[k + 1]); a record's ctg is its index there.  Resets both sides.
 * _set_regions: the confident regions, sorted and merged per contig, 0-based half-open: those of contig k are [first[k], first[k + 1])
 *   of starts / ends, first [n_contigs + 1]; n_intervals < 0: none, everything is inside.
 * _parse: stats [8] = lines, data rows, records, the drop counters symbolic, unknown_contig, too_long, sorted (1: the records are in
 *   (contig, pos) order as they stand), 0.  Returns non-zero for a malformed row, with a message that names the side and the 1-based line.
 * _keys: the 8-byte key (ctg << 32 | pos) of every record, in the order the records have.  _permute: record i becomes what record perm[i]
 *   was (the stable permutation the host sorted the keys with).  _run refuses a side that is not in order.
 * _run: duplicates, regions, join, the counters and the suffix sums.  _counts: CLAIR_COMPARE_COUNTS int64, laid out as the table in
 *   docs/compare_vcf.md (counts [2][4][6], hist [4][3][1024], at_least [4][3][1024], drops [2][3]).
 * _records: the records of a side and one outcome byte each (0 TP, 1 GT, 2 FP, 3 FN, 4 DUP, 5 OUTSIDE); either array may be NULL.
 * Every call is synchronous.  Non-zero on failure, message from clair_compare_last_error (NULL handle: the failure of create).
 * clair_host_compare_* (include/clair_host.h) gives the same integers on the CPU. */
#define CLAIR_COMPARE_COUNTS 24630
typedef struct clair_compare clair_compare_t;
#ifndef CLAIR_COMPARE_RECORD_T
#define CLAIR_COMPARE_RECORD_T
typedef struct clair_compare_record clair_compare_record_t;
#endif
int clair_compare_create(int device, clair_compare_t **out);
void clair_compare_destroy(clair_compare_t *h);
const char *clair_compare_last_error(const clair_compare_t *h);
int clair_compare_set_contigs(clair_compare_t *h, const uint8_t *names, const int64_t *offsets, int n_contigs);
int clair_compare_set_regions(clair_compare_t *h, const int64_t *first, const int64_t *starts, const int64_t *ends, int64_t n_intervals);
int clair_compare_parse(clair_compare_t *h, int side, const uint8_t *text, int64_t len, int64_t *stats);
int clair_compare_keys(clair_compare_t *h, int side, int64_t *keys);
int clair_compare_permute(clair_compare_t *h, int side, const int64_t *perm);
int clair_compare_run(clair_compare_t *h);
int clair_compare_counts(clair_compare_t *h, int64_t *counts);
int clair_compare_records(clair_compare_t *h, int side, clair_compare_record_t *records, uint8_t *outcomes);
/* Left alignment of indels (compare_vcf --left_align; docs/compare_vcf.md, "Left alignment"), opt-in: without these calls nothing changes.
 * _set_reference: the sequences of the contig table one after the other, contig k = seq[offsets[k] .. offsets[k + 1]), offsets
 *   [n_contigs + 1] with n_contigs that of _set_contigs; an empty range: no sequence for that contig.  Copied to the device.  Any time after
 *   _set_contigs and before _left_align.
 * _left_align: after _parse of that side, before _keys / _permute / _run, once per parse.  Every record's alleles go upper-cased to an
 *   allele arena the handle owns (record i of the order they have at slot sum_{j<i} (ref_len_j + alt_len_j), REF first), indels move to
 *   their leftmost position, and from here on ref_off / alt_off index the arena.  stats [8] = examined, shifted, ref_mismatch,
 *   at_contig_start, no_sequence, sorted (the order flag on the new positions: it supersedes _parse's), arena bytes, 0.
 * _allele_text: the arena of a left-aligned side (stats[6] bytes). */
int clair_compare_set_reference(clair_compare_t *h, const uint8_t *seq, const int64_t *offsets, int n_contigs);
int clair_compare_left_align(clair_compare_t *h, int side, int64_t *stats);
int clair_compare_allele_text(clair_compare_t *h, int side, uint8_t *out);

/* ---- index_bam: the .bai of a coordinate-sorted BAM, built on the device (csrc/bam_index.hip; docs/index_bam.md) ----
 * One handle: one stream, the device buffers of a batch and the linear index.  segment_bytes: the framing segment, a power of two in
 * 64 .. 8192, 0 for the default (8192).
 * _begin: a new file with n_ref references of ref_len bases; the linear index (one uint64 per 16 KiB window of every reference, a
 *   reference's windows after those of the one before it) is set to all-ones, the counters and the carried bytes are dropped.
 * _batch: n <= max_blocks whole BGZF blocks (block i = cdata[in_at[i] .. + csize[i]), out_len[i] its ISIZE, coffset[i] its offset in the
 *   file; end_coffset that of the block after the batch), whose headers the caller has walked.  The blocks are inflated behind the bytes the
 *   batch before carried over, into one device buffer that never comes back; records are framed from `entry` (an offset into that stream: where
 *   the first record starts), their fields, virtual offsets, runs and linear-index minima computed there.  Back come only the runs (*runs:
 *   state[4] of them, the handle's until the next call) and state (CLAIR_BAMIDX_STATE).  The bytes from the first record that does not end
 *   inside the batch are carried to the next; with last != 0 such bytes are an error.  The caller joins a batch's first run to the last of
 *   the batch before when tid, bin and the offsets meet.
 * _finish: the linear index (n_windows as _begin laid it out; all-ones: untouched) and counts [3] = records, mapped, unplaced.
 * _backend: the three calls above with the handle, as clair_host_bamidx_build takes them.
 * _debug_frame: the framing alone on a host byte stream (tests): starts [cap], result [4] = starts, tail, bad (the chain hit a
 *   block_size that cannot be), sentinels intact (words behind the stream and behind the offsets array, checked after the kernels).
 * Non-zero on failure, message from clair_bamidx_last_error (NULL handle: the failure of create); a failed batch leaves the handle fit for
 * _begin.  clair_host_bamidx_* (include/clair_host.h) gives the same bytes on the CPU. */
typedef struct clair_bamidx clair_bamidx_t;
#ifndef CLAIR_BAMIDX_TYPES
#define CLAIR_BAMIDX_TYPES
/* one run of records next to each other in the file that share (tid, bin): one chunk of a .bai, [beg, end) as virtual offsets */
typedef struct clair_bamidx_run {
    int32_t tid;
    uint32_t bin;
    uint64_t beg, end;
} clair_bamidx_run_t;      /* 24 bytes */
/* the batch interface of an index build, as the file driver (clair_host_bamidx_build) calls it: the entry points of one backend with its handle */
typedef struct clair_bamidx_backend {
    void *ctx;
    int (*begin)(void *ctx, int n_ref, const int64_t *ref_len);
    int (*batch)(void *ctx, const uint8_t *cdata, int64_t cbytes, int n, const int64_t *in_at, const int32_t *csize, const int32_t *out_len,
                 const int64_t *coffset, int64_t end_coffset, int64_t entry, int last, int64_t *state, const clair_bamidx_run_t **runs);
    int (*finish)(void *ctx, uint64_t *linear, int64_t n_windows, int64_t *counts);
    const char *(*last_error)(const void *ctx);
} clair_bamidx_backend_t;
#define CLAIR_BAMIDX_STATE 8   /* int64 words of `state`: in 0 records before the batch, 1 2 tid and pos of the record before it (0, INT32_MIN: none);
                                * out 3 records, 4 runs, 5 6 tid and pos of the last record (1 2 when there is none), 7 bytes carried over */
#endif
int clair_bamidx_create(int device, int max_blocks, int segment_bytes, clair_bamidx_t **out);
void clair_bamidx_destroy(clair_bamidx_t *h);
const char *clair_bamidx_last_error(const clair_bamidx_t *h);
int clair_bamidx_begin(clair_bamidx_t *h, int n_ref, const int64_t *ref_len);
int clair_bamidx_batch(clair_bamidx_t *h, const uint8_t *cdata, int64_t cbytes, int n, const int64_t *in_at, const int32_t *csize, const int32_t *out_len,
                       const int64_t *coffset, int64_t end_coffset, int64_t entry, int last, int64_t *state, const clair_bamidx_run_t **runs);
int clair_bamidx_finish(clair_bamidx_t *h, uint64_t *linear, int64_t n_windows, int64_t *counts);
int clair_bamidx_backend(clair_bamidx_t *h, clair_bamidx_backend_t *out);
int clair_bamidx_debug_frame(clair_bamidx_t *h, const uint8_t *stream, int64_t n, int64_t entry, int64_t *starts, int64_t cap, int64_t *result);

/* ---- sort_bam: a BAM sorted by coordinate on the device (csrc/bam_sort.hip; docs/sort_bam.md) ----
 * One handle: one stream, the device buffers of a batch (those of index_bam's batch front), the group buffer, the sorted buffer and the
 * byte histogram.  The key of a record is (uint32)tid << 32 | (uint32)(pos + 1) << 1 | reverse strand; equal keys keep their input order.
 * _begin: a new file with n_ref references of ref_len bases; memory: the most record bytes a group may hold.  The histogram has one bucket
 *   per 2^20 positions of every reference (at least one each) and a last one for the records without a reference.
 * _pass: a new read of the input: records whose bucket lies in [bucket_lo, bucket_hi) are kept.  first != 0: the histogram is counted and a
 *   group that outgrows `memory` is dropped and reported (state[7]) instead of refused.
 * _batch: n <= max_blocks whole BGZF blocks, as clair_bamidx_batch takes them.  Inflated, framed, every record's key, length and bucket
 *   computed on the device, the kept ones compacted behind the group's records.  Back comes only state (CLAIR_BAMSORT_STATE).
 * _histogram: bytes of records per bucket, as the first read counted them.
 * _sort: the group sorted (stable LSD radix sort, 8 bits a pass, passes whose digit is the same in every key skipped) and gathered behind
 *   the bytes the group before left over; info (CLAIR_BAMSORT_INFO).  last == 0: the bytes behind the last whole payload of 65280 are kept
 *   for the next group; last != 0: they are a payload of their own.
 * _emit: payloads [first, first + n) of the sorted buffer, n <= 64.  compressed != 0: deflate_bgzf_kernel over the device-resident bytes,
 *   block i in out[i * 65536 .. + sizes[i]); compressed == 0: the bytes themselves, packed, sizes[i] bytes each.
 * _backend: the calls above with the handle, as clair_host_bamsort_run takes them.
 * _debug_sort: the radix sort alone: perm [n] = the stable order of keys [n].  _debug_gather: the gather alone: the records at starts [n] of
 *   `stream` in the order perm into out[0 .. out_bytes), which must be their total length; a guard region in front of and behind the device's
 *   output is checked after the kernel.
 * Non-zero on failure, message from clair_bamsort_last_error (NULL handle: the failure of create).  clair_host_bamsort_* (include/clair_host.h)
 * gives the same bytes on the CPU. */
typedef struct clair_bamsort clair_bamsort_t;
#ifndef CLAIR_BAMSORT_TYPES
#define CLAIR_BAMSORT_TYPES
/* the interface of a sort, as the file driver (clair_host_bamsort_run) calls it: the entry points of one backend with its handle */
typedef struct clair_bamsort_backend {
    void *ctx;
    int (*begin)(void *ctx, int n_ref, const int64_t *ref_len, int64_t memory);
    int (*pass)(void *ctx, int64_t bucket_lo, int64_t bucket_hi, int first);
    int (*batch)(void *ctx, const uint8_t *cdata, int64_t cbytes, int n, const int64_t *in_at, const int32_t *csize, const int32_t *out_len,
                 const int64_t *coffset, int64_t end_coffset, int64_t entry, int last, int64_t *state);
    int (*histogram)(void *ctx, int64_t *bytes, int64_t n_buckets);
    int (*sort)(void *ctx, int last, int64_t *info);
    int (*emit)(void *ctx, int64_t first, int n, int compressed, uint8_t *out, int32_t *sizes);
    const char *(*last_error)(const void *ctx);
} clair_bamsort_backend_t;
#define CLAIR_BAMSORT_STATE 11 /* int64 words of `state`: in 0 records before the batch, 1 the key of the record before it (0: none); out 2 records,
                                * 3 the last record's key (1 when there is none), 4 5 records and bytes kept for the group, 6 a record came before
                                * its predecessor, 7 the group outgrew `memory` and was dropped (first read only), 8 9 mapped and unplaced records,
                                * 10 bytes carried over */
#define CLAIR_BAMSORT_INFO 4   /* int64 words of _sort's `info`: bytes in the sorted buffer, payloads ready for _emit, records sorted, radix passes run */
#define CLAIR_BAMSORT_STATS 7  /* of clair_host_bamsort_run: records, mapped, unplaced, groups, reads of the input, already sorted, bytes appended */
#endif
int clair_bamsort_create(int device, int max_blocks, int segment_bytes, clair_bamsort_t **out);
void clair_bamsort_destroy(clair_bamsort_t *h);
const char *clair_bamsort_last_error(const clair_bamsort_t *h);
int clair_bamsort_begin(clair_bamsort_t *h, int n_ref, const int64_t *ref_len, int64_t memory);
int clair_bamsort_pass(clair_bamsort_t *h, int64_t bucket_lo, int64_t bucket_hi, int first);
int clair_bamsort_batch(clair_bamsort_t *h, const uint8_t *cdata, int64_t cbytes, int n, const int64_t *in_at, const int32_t *csize, const int32_t *out_len,
                        const int64_t *coffset, int64_t end_coffset, int64_t entry, int last, int64_t *state);
int clair_bamsort_histogram(clair_bamsort_t *h, int64_t *bytes, int64_t n_buckets);
int clair_bamsort_sort(clair_bamsort_t *h, int last, int64_t *info);
int clair_bamsort_emit(clair_bamsort_t *h, int64_t first, int n, int compressed, uint8_t *out, int32_t *sizes);
int clair_bamsort_backend(clair_bamsort_t *h, clair_bamsort_backend_t *out);
int clair_bamsort_debug_sort(clair_bamsort_t *h, const uint64_t *keys, int64_t n, uint32_t *perm);
int clair_bamsort_debug_gather(clair_bamsort_t *h, const uint8_t *stream, int64_t stream_bytes, const int64_t *starts, const uint32_t *perm, int64_t n,
                               uint8_t *out, int64_t out_bytes);

/* ---- markdup_bam: duplicate reads flagged (0x400) or removed on the device (csrc/markdup.hip; docs/markdup_bam.md) ----
 * One handle: one stream, the device buffers of a batch (those of index_bam's batch front), one 32-byte summary per record of the file
 * (clair_markdup_summary_t), the buffers of the resolution (the radix sort of sort_bam) and the output of the second read.
 * _begin: a new file with n_ref references; memory: the most bytes the summaries may hold; remove != 0: the second read drops the records
 *   the rule flagged instead of writing them.
 * _batch: the first read.  n <= max_blocks whole BGZF blocks, as clair_bamidx_batch takes them: inflated, framed, every record summarised on
 *   the device (end, name hash, score, bits, index).  Back comes only state (CLAIR_MARKDUP_STATE).
 * _resolve: the rule over the summaries -> one byte per record on the device, 1: duplicate.  No atomic decides an order: stable radix sorts
 *   and neighbour comparisons only, so two runs give the same bytes.
 * _mark: the second read, the same batches in the same order.  Bit 0x400 of every examined record set or cleared where it lies, then the
 *   batch's records (remove: those kept, compacted) put behind the bytes the batch before left over; info (CLAIR_MARKDUP_INFO).  last == 0:
 *   the bytes behind the last whole payload of 65280 are kept for the next batch; last != 0: they are a payload of their own.
 * _emit: payloads [first, first + n) of that buffer, n <= 64, as clair_bamsort_emit hands them out.
 * _stats: counts [CLAIR_MARKDUP_COUNTS] of the resolution.
 * _backend: the calls above with the handle, as clair_host_markdup_run takes them.
 * _debug_summary: the summaries of the n records at `starts` of a raw record stream (every start checked on the host first).
 * _debug_resolve: the resolution alone over n given summaries -> duplicate [n].
 * _debug_mark: the second read's kernels alone over n back-to-back records of a raw stream with given summaries and duplicate bytes ->
 *   patched_stream [stream_bytes] and the records written (remove != 0: compacted) in out, which has room for all n; *out_bytes their
 *   length.  Guard regions in front of and behind the device's stream and output are checked after the kernels.
 * Non-zero on failure, message from clair_markdup_last_error (NULL handle: the failure of create).  clair_host_markdup_* (include/clair_host.h)
 * gives the same bytes on the CPU. */
typedef struct clair_markdup clair_markdup_t;
#ifndef CLAIR_MARKDUP_TYPES
#define CLAIR_MARKDUP_TYPES
typedef struct clair_markdup_summary {
    uint64_t end;   /* tid << 33 | (unclipped 5' position + 2^31) << 1 | reverse strand; all ones: the record is not examined */
    uint64_t hash;  /* FNV-1a (64 bit) of the read name without its NUL */
    uint32_t score; /* sum of the base qualities >= 15, clamped */
    uint32_t index; /* of the record in the file */
    uint32_t bits;  /* 1 examined, 2 can have a mate, 4 read 2 (else read 1), 8 reverse strand */
    uint32_t pad;
} clair_markdup_summary_t;
/* the interface of the stage, as the file driver (clair_host_markdup_run) calls it: the entry points of one backend with its handle */
typedef struct clair_markdup_backend {
    void *ctx;
    int (*begin)(void *ctx, int n_ref, int64_t memory, int remove);
    int (*batch)(void *ctx, const uint8_t *cdata, int64_t cbytes, int n, const int64_t *in_at, const int32_t *csize, const int32_t *out_len,
                 const int64_t *coffset, int64_t end_coffset, int64_t entry, int last, int64_t *state);
    int (*resolve)(void *ctx);
    int (*mark)(void *ctx, const uint8_t *cdata, int64_t cbytes, int n, const int64_t *in_at, const int32_t *csize, const int32_t *out_len,
                const int64_t *coffset, int64_t end_coffset, int64_t entry, int last, int64_t *info);
    int (*emit)(void *ctx, int64_t first, int n, int compressed, uint8_t *out, int32_t *sizes);
    int (*stats)(void *ctx, int64_t *counts);
    const char *(*last_error)(const void *ctx);
} clair_markdup_backend_t;
#define CLAIR_MARKDUP_STATE 3  /* int64 words of _batch's `state`: records summarised so far, records of this batch, bytes carried over */
#define CLAIR_MARKDUP_INFO 4   /* of _mark's `info`: bytes in the output buffer, payloads ready for _emit, records of this batch, records written */
#define CLAIR_MARKDUP_COUNTS 6 /* of _stats: records, examined, pairs, fragments, duplicate pairs, duplicate fragments */
#define CLAIR_MARKDUP_STATS 9  /* of clair_host_markdup_run: the six counts, duplicate records, records written, bytes appended */
#endif
int clair_markdup_create(int device, int max_blocks, int segment_bytes, clair_markdup_t **out);
void clair_markdup_destroy(clair_markdup_t *h);
const char *clair_markdup_last_error(const clair_markdup_t *h);
int clair_markdup_begin(clair_markdup_t *h, int n_ref, int64_t memory, int remove);
int clair_markdup_batch(clair_markdup_t *h, const uint8_t *cdata, int64_t cbytes, int n, const int64_t *in_at, const int32_t *csize, const int32_t *out_len,
                        const int64_t *coffset, int64_t end_coffset, int64_t entry, int last, int64_t *state);
int clair_markdup_resolve(clair_markdup_t *h);
int clair_markdup_mark(clair_markdup_t *h, const uint8_t *cdata, int64_t cbytes, int n, const int64_t *in_at, const int32_t *csize, const int32_t *out_len,
                       const int64_t *coffset, int64_t end_coffset, int64_t entry, int last, int64_t *info);
int clair_markdup_emit(clair_markdup_t *h, int64_t first, int n, int compressed, uint8_t *out, int32_t *sizes);
int clair_markdup_stats(clair_markdup_t *h, int64_t *counts);
int clair_markdup_backend(clair_markdup_t *h, clair_markdup_backend_t *out);
int clair_markdup_debug_summary(clair_markdup_t *h, const uint8_t *stream, int64_t stream_bytes, const int64_t *starts, int64_t n, int n_ref,
                                clair_markdup_summary_t *out);
int clair_markdup_debug_resolve(clair_markdup_t *h, const clair_markdup_summary_t *summaries, int64_t n, uint8_t *duplicate);
int clair_markdup_debug_mark(clair_markdup_t *h, const uint8_t *stream, int64_t stream_bytes, const int64_t *starts, int64_t n,
                             const clair_markdup_summary_t *summaries, const uint8_t *duplicate, int remove, uint8_t *patched_stream, uint8_t *out,
                             int64_t *out_bytes);

#ifdef __cplusplus
}
#endif
#endif /* CLAIR_AMD_H */
