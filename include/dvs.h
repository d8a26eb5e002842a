/* dvs.h — C ABI of libdvs_hip.so: the MI355X-native PACE-VAE train-step hot path.
 *
 * The reference (rlog58/dags-vae-search) is 100 % Python and has no FFI of its own: its boundary for this
 * path is the Python class surface of PaceVaeV3 (src/encoders/pace.py:1139-2046) and train_batch
 * (experiments/03_synthetic_12/main.py:95-118).  This header is the C ABI that sits UNDER the drop-in
 * Python mirror (dags_vae_search_amd/pace.py, train.py); each entry point cites the reference code it
 * replaces.  INTEGRATION.md shows the ctypes binding.
 *
 * Conventions: plain pointers and sizes only (no torch types).  Every pointer marked "device" is device
 * memory owned by the caller; the library never allocates or frees device memory and never synchronises
 * the host with the device.  All work is enqueued on the passed HIP stream (void* = hipStream_t).
 * Return value: 0 = ok, non-zero = error code; dvs_last_error() gives the thread-local message.  Codes: 1-5 bad shape,
 * 10 null pointer, 12/13 bad argument, 14 a caller buffer is smaller than the shape needs (records_bytes, n_params,
 * workspace_bytes, state_bytes are checked against dvs_record_bytes / dvs_param_count / dvs_workspace_bytes BEFORE anything
 * is enqueued), 20 the HIP runtime refused a kernel launch or an attribute/copy call of this entry point (message names
 * the kernel and carries hipGetErrorString; work enqueued before the failing launch stays enqueued, results are undefined).
 * Entry points are re-entrant: the only process-global state is the optional profiler record (dvs_profile_*), which is
 * mutex-guarded; error state is thread-local.
 *
 * Fixed architecture of this build (BASELINE.json configs; experiments/01_bn_asia/main.py:33-43):
 * vertices_embedding_size 32, num_heads 8, num_layers 3, ff_hidden_size 64, latent_layer_size 32,
 * fc_hidden 32.  n_tokens = n + 3 <= 48, n_classes = card + 3 <= 48.  Shapes with n_tokens <= 16 and n_classes <= 16
 * (asia, sachs, n = 12) take the one-tile path (a wavefront owns a DAG); larger ones (alarm-size, n = 37) the tiled
 * "wide" path (a workgroup owns a DAG, tiles of 16 tokens meet in LDS).  Same entry points for both.
 */
#ifndef DVS_H
#define DVS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DVS_VERSION 202
#define DVS_NUM_PARAMS 108
#define DVS_RECORD_BYTES 96          /* one-tile path */
#define DVS_RECORD_BYTES_WIDE 864    /* wide path; dvs_record_bytes(shape) returns the one that applies */
#define DVS_CLIP_SCRATCH_FLOATS 4096  /* 2 + partial sums of squares: 256 (dvs_clip_adam) or one per 256 parameters (dvs_loss_backward_sq) */
#define DVS_DECODE_STATE_BYTES 440   /* sizeof(dvs_decode_state) */

typedef struct dvs_shape {
    int32_t batch;        /* DAGs in this (rank-local) batch */
    int32_t n_tokens;     /* N = max_num_vertices + 3 (pace.py:1159), <= 48 */
    int32_t n_classes;    /* C = vertex_label_cardinality + 3 (pace.py:1160), <= 48 */
    int32_t training;     /* 1 = model.train(): dropout + reparameterisation noise; 0 = eval */
    float dropout;        /* p of every nn.Dropout / attention dropout (pace.py:1150) */
    float beta;           /* KL weight (pace.py:1977) */
    float eps_scale;      /* epsilon_scale of reparameterize (pace.py:1653), 0.01 */
    uint32_t dag_offset;  /* global index of this batch's first DAG (data-parallel shard offset) */
    uint64_t seed;        /* counter-based RNG seed; fold the step number in on the host */
} dvs_shape;

typedef struct dvs_param_entry {
    char name[64];        /* reference state-dict key, e.g. "encoder.layers.0.self_attn.in_proj_weight" */
    int64_t offset;       /* float offset inside the flat parameter / gradient buffer (16-byte aligned) */
    int32_t rows, cols;   /* cols == 0 for 1-D tensors */
} dvs_param_entry;

int dvs_version(void);
const char* dvs_last_error(void);
int dvs_device_cus(void);   /* compute units of the current device (grid sizing; informational) */

/* Flat parameter buffer: the 108 tensors of PaceVaeV3.state_dict() (pace.py:1176-1207) in registration
 * order, each 16-byte aligned.  dvs_param_table fills up to `cap` entries and returns the count. */
int64_t dvs_param_count(const dvs_shape* s);
int dvs_param_table(const dvs_shape* s, dvs_param_entry* out, int cap);

/* Scratch needed by forward+backward for s->batch DAGs (saved activations, gradient slabs). */
size_t dvs_workspace_bytes(const dvs_shape* s);

/* Bytes of one compact per-DAG record for this shape (96 or 864); the caller allocates batch * this. */
size_t dvs_record_bytes(const dvs_shape* s);

/* Replaces the `.to(device)` feature hand-over at pace.py:1981-1985 / 1616-1619: reads the reference-layout
 * dense features — vertex_label_features [B,N,C] f32, vertex_position_features [B,N,N] f32,
 * adjacency_matrices [B,N,N] f32, target_masks [8B,N,N] bool (1 byte each) — and writes one compact record
 * (dvs_record_bytes) per DAG.  status (device int32[1], zeroed by the caller) gets bit 0 set if a label/position
 * row is not one-hot, bit 1 if the 8 per-head masks of a DAG differ, bit 2 if a mask row forbids self. */
int dvs_pack_features(const dvs_shape* s, const float* label_onehot, const float* pos_onehot,
                      const float* adjacency, const uint8_t* target_masks, void* records, size_t records_bytes,
                      int32_t* status, void* stream);

/* Device-side feature front-end (replaces LabeledDag.from_dict_to_graph src/toolkit/labeled.py:132-154 +
 * from_labeled_graph_to_pace_graph pace.py:1250-1288 + generate_mask 1307-1343 + prepare_features 1345-1478 + pack):
 * builds the records straight from the row codec.  labels: device u8 [B][n] (n = n_tokens - 3, l{v} columns);
 * preds: device [B][n], bit u of preds[b][v] set <=> edge u -> v (the e{v} '0/1' string, u < v); element type u16 on
 * the one-tile path (dvs_record_bytes == 96), u64 on the wide path.  One thread per DAG does the PACE wrapping, the
 * FIFO-Kahn topological order (positions[v] = order[v], the reference's quirk), and the ancestor closure on bit rows.  status bit 0: a label is >= n_classes - 3; bit 3: an edge with u >= v. */
int dvs_build_records(const dvs_shape* s, const uint8_t* labels, const void* preds, void* records, size_t records_bytes,
                      int32_t* status, void* stream);

/* Buffer sizes: every compute entry point takes the byte size of the record buffer (>= batch * dvs_record_bytes), the
 * float count of the flat parameter (and gradient) buffer (>= dvs_param_count) and the byte size of the workspace
 * (>= dvs_workspace_bytes) and returns 14 without enqueueing anything when one is too small. */

/* PaceVaeV3.loss_direct forward (pace.py:1974-2035).  eps: optional device [B,32] noise already multiplied
 * by eps_scale (NULL = counter-based normal draws when training).  losses (device f32[DVS_LOSS_FLOATS = 5]):
 * {total, recon = -log-likelihood, kld, non-finite flag, invalid-features flag}.  status: optional device int32[1], the
 * validation word of the dvs_pack_features / dvs_build_records call that wrote `records`; losses[4] = 1 if it is
 * non-zero (0 when status is NULL), so that the flag can travel with the loss scalars (data-parallel all-reduce,
 * dvs_clip_adam's guard).  mu/logvar: optional device [B,32] outputs. */
#define DVS_LOSS_FLOATS 5
int dvs_loss_forward(const dvs_shape* s, const void* records, size_t records_bytes, const float* params, int64_t n_params,
                     void* workspace, size_t workspace_bytes, const float* eps, const int32_t* status, float* losses,
                     float* mu, float* logvar, void* stream);

/* dvs_loss_forward that also tells the HOST when the loss scalars are final, without an event or a copy on any stream (ABI 201).
 * host_tail: 16 bytes (16-byte aligned) of pinned, device-mapped host memory (hipHostMalloc / torch pin_memory).  The kernel
 * that reduces the per-DAG losses writes them with ONE 16-byte store: [0] total, [1] recon, [2] kld (f32), [3] a uint32 word
 * = (host_seq << 8) | (invalid-features flag << 7) | (non-finite flag << 6) | (validation word *status & 0x3F).  A host that
 * polls word [3] until its upper 24 bits equal the host_seq it passed (24 bits are kept), and reads [0..2] AFTER that, has final
 * values where the reference's `loss.item()` returns (experiments/03_synthetic_12/main.py:104), while backward and optimiser
 * are still queued.  With host_tail the validation word is RE-ARMED (*status = 0) once it has been read: status is written.
 * Coherence REQUIREMENT on host_tail (the library cannot check it): fine-grained / coherent pinned memory — what
 * hipHostMalloc gives by default (hipHostMallocCoherent) and what torch.pin_memory() allocates —, uncached on the device, so
 * that the single 16-byte store becomes one PCIe write the host sees whole; memory registered non-coherent
 * (hipHostMallocNonCoherent, hipExtHostRegisterCoarseGrained) is only guaranteed visible at the end of the kernel and must
 * not be used.  A careful host re-reads word [3] AFTER reading [0..2] and retries when it changed (the Python driver does);
 * a host that cannot rely on this passes host_tail = NULL and waits for an event instead (DVS_EARLY_READ=event). */
int dvs_loss_forward_notify(const dvs_shape* s, const void* records, size_t records_bytes, const float* params,
                            int64_t n_params, void* workspace, size_t workspace_bytes, const float* eps, int32_t* status,
                            float* losses, float* mu, float* logvar, void* host_tail, uint32_t host_seq, void* stream);

/* Backward of the same step (autograd of pace.py:1974-2035; experiments/03_synthetic_12/main.py:114).  Must follow
 * dvs_loss_forward on the same workspace and parameters: it reads the forward's saved activations and per-step weight images.
 * gcoef (device f32[2]): d(objective)/d(recon), d(objective)/d(kld).  grads: flat buffer, overwritten. */
int dvs_loss_backward(const dvs_shape* s, const void* records, size_t records_bytes, const float* params, int64_t n_params,
                      void* workspace, size_t workspace_bytes, const float* gcoef, float* grads, void* stream);

/* dvs_loss_backward that also leaves the partial sums of squares of `grads` — one per 256 gradient entries, written by the
 * kernel that sums the gradient slabs, in a fixed order — in clip_scratch[2 ..] (device f32[DVS_CLIP_SCRATCH_FLOATS], the
 * `scratch` of the dvs_clip_adam_from_partials call that follows; NULL: plain dvs_loss_backward).  (ABI 202.)  For the
 * single-process step only: clip_grad_norm_ (experiments/03_synthetic_12/main.py:115) needs the norm of the gradient the
 * optimiser sees, so a data-parallel step, whose gradient changes in the all-reduce, uses dvs_loss_backward + dvs_clip_adam. */
int dvs_loss_backward_sq(const dvs_shape* s, const void* records, size_t records_bytes, const float* params, int64_t n_params,
                         void* workspace, size_t workspace_bytes, const float* gcoef, float* grads, float* clip_scratch,
                         void* stream);

/* The fused single-process train step with the loss head run ONCE (one-tile path, n_tokens and n_classes <= 16; 13 otherwise).
 * The loss-head backward recomputes every quantity of the loss-head forward — logits, their maximum and sum of exponentials,
 * all pair logits — and needs no loss value (its only coefficient is gcoef), so the pair below leaves the forward's loss-head
 * launch out and lets the backward's write the per-DAG reconstruction loss.  Additions to ABI 202; the version number stays.
 *   dvs_loss_forward_defer: dvs_loss_forward up to and including the decoder (per-DAG KL terms, saved activations, weight
 *     images, optional mu / logvar); it writes NO loss scalars.
 *   dvs_loss_backward_emit: dvs_loss_backward_sq whose first kernel also writes the per-DAG reconstruction loss, followed at
 *     once by the reduction to `losses` (as dvs_loss_forward defines them; the guard of the dvs_clip_adam* call behind it may
 *     point at &losses[3]) and, with host_tail, by the host notification of dvs_loss_forward_notify — same packet, same
 *     coherence requirement, same re-arming of *status —, which the host now sees one kernel later than behind a forward.
 *     losses == NULL: exactly dvs_loss_backward_sq (status, host_tail, host_seq unused; must then follow dvs_loss_forward*).
 * Gradients are bit-identical to dvs_loss_forward + dvs_loss_backward_sq.  The reconstruction loss is the same sum of the same
 * terms with the pair logits taken from the backward's recompute, whose 64-term inner sum is associated differently: it
 * agrees with dvs_loss_forward's to fp32 rounding, not bit for bit; kld, mu, logvar are bit-identical. */
int dvs_loss_forward_defer(const dvs_shape* s, const void* records, size_t records_bytes, const float* params,
                           int64_t n_params, void* workspace, size_t workspace_bytes, const float* eps, float* mu,
                           float* logvar, void* stream);
int dvs_loss_backward_emit(const dvs_shape* s, const void* records, size_t records_bytes, const float* params,
                           int64_t n_params, void* workspace, size_t workspace_bytes, const float* gcoef, float* grads,
                           float* clip_scratch, int32_t* status, float* losses, void* host_tail, uint32_t host_seq,
                           void* stream);

/* PaceVaeV3.encode_direct (pace.py:1613-1641): mu, logvar device [B,32]. */
int dvs_encode(const dvs_shape* s, const void* records, size_t records_bytes, const float* params, int64_t n_params,
               void* workspace, size_t workspace_bytes, float* mu, float* logvar, void* stream);

/* clip_grad_norm_(params, max_norm) + Adam.step (experiments/03_synthetic_12/main.py:115-116, lr 1e-4,
 * betas (0.9, 0.999), eps 1e-8, no weight decay) over flat buffers of n floats.  max_norm <= 0 disables
 * clipping.  scratch: device f32[DVS_CLIP_SCRATCH_FLOATS] ([0] = sum of squares, [1] = clip coefficient, rest =
 * partial sums); `step` is the 1-based Adam step.  guard: optional device f32[2] (normally &losses[3] of the step's
 * dvs_loss_forward, after the data-parallel all-reduce): when guard[0] != 0 (non-finite loss) or guard[1] != 0 (invalid
 * features) the whole update is skipped on the device — params, exp_avg, exp_avg_sq and grads stay as they are, as in the
 * reference, where loss_direct raises before backward / clip / step run (pace.py:97-98, main.py:111-116). */
int dvs_clip_adam(int64_t n, float* params, float* grads, float* exp_avg, float* exp_avg_sq, float lr,
                  float beta1, float beta2, float adam_eps, int64_t step, float max_norm, float* scratch,
                  const float* guard, void* stream);

/* The same update from the partial sums of squares dvs_loss_backward_sq left in scratch[2 ..] for exactly these n gradient
 * entries (one launch instead of two: no pass over the gradient for its norm).  (ABI 202.) */
int dvs_clip_adam_from_partials(int64_t n, float* params, float* grads, float* exp_avg, float* exp_avg_sq, float lr,
                                float beta1, float beta2, float adam_eps, int64_t step, float max_norm, float* scratch,
                                const float* guard, void* stream);

/* One grown PACE graph of dvs_decode (vertex 0 = start, 1 = input, then the sampled vertices in order). */
typedef struct dvs_decode_state {
    uint64_t parents[48];   /* bit j of parents[i]: edge j -> i */
    uint8_t label[48];      /* PACE label of vertex i (user label + 3; 0 input, 1 output, 2 start) */
    int32_t nv;             /* number of vertices; == n_tokens unless the graph sampled `output` early */
    int32_t finished;       /* 1: the graph sampled `output` and stopped growing (pace.py:1738-1743) */
} dvs_decode_state;

/* PaceVaeV3.decode (pace.py:1666-1749), batched on the device.  z: device [B,32] latents;
 * records: device scratch of batch * dvs_record_bytes bytes; state_out: device dvs_decode_state[B].  The whole
 * n_tokens - 2 step autoregressive loop (records of the partial graphs -> embedding -> 3 decoder layers -> node-type /
 * edge sampling -> graph update) is enqueued on `stream`; nothing is read back in between.  uniforms: optional device
 * f32 [B, n_tokens, n_tokens]; step idx uses [b, idx, 0] for the node type (inverse CDF, as np.random.choice) and
 * [b, idx, 1 + vi] for edge candidate vi (edge iff u < sigmoid score, as torch.rand_like < score); NULL = counter-based
 * draws from s->seed.  s->training must be 0 (the reference decodes in eval mode). */
int dvs_decode(const dvs_shape* s, const float* params, int64_t n_params, void* workspace, size_t workspace_bytes,
               void* records, size_t records_bytes, const float* z, const float* uniforms, void* state_out,
               size_t state_bytes, void* stream);

/* Reconstruction judging of decoded rows (the toolkit.is_valid_graph / graph_equals loop of batch_test,
 * experiments/03_synthetic_12/main.py:200-217) on the device.  Targets in the row codec of dvs_build_records: labels device u8
 * [batch][n_vars], preds device [batch][n_vars] (u16, or u64 when preds_are_u64; bit u of preds[v] <=> edge u -> v); states:
 * device dvs_decode_state [batch * repeats] as dvs_decode leaves them, row k decoded from target k / repeats (user vertex i =
 * PACE vertex i + 2, label - 3, edge u -> v (u < v) <=> bit u + 2 of parents[v + 2]).  flags: device u8 [batch * repeats],
 * bit 0 valid (nv == n_vars + 3 and every label in [0, card)), bit 1 isomorphic ignoring labels, bit 2 label-preserving
 * isomorphic, bit 3 undecided (an exact search visited more than `budget` nodes; bits 1-2 are then unspecified).  A row with
 * nv < n_vars + 3 gets 0.  Exact: "isomorphic" only from a verified complete mapping, "not isomorphic" only from an
 * isomorphism invariant (colour refinement) or an exhausted search.  1 <= n_vars, card <= 45; batch * repeats <= 2^30.
 * (Added in ABI 202 as a pure addition: the version number stays.) */
int dvs_match_decoded(int32_t batch, int32_t n_vars, int32_t card, int32_t repeats, int32_t preds_are_u64,
                      const uint8_t* labels, const void* preds, const void* states, size_t state_bytes,
                      int32_t budget, uint8_t* flags, void* stream);

/* Search candidates on the device (dags_vae_search_amd/search.py, candidates="device"; csrc/dvs_structs.h): what the host
 * stage between decode and BIC computes per decoded row (graphs_from_states -> is_search_valid -> encode_graphs ->
 * structure_key), for states: device dvs_decode_state [batch] as dvs_decode leaves them (same vertex / edge convention as
 * dvs_match_decoded; edges go from a lower to a higher vertex, so a row is acyclic by construction).
 * flags: device u8 [batch], bit 0 search-valid: nv == n_vars + 3 and the user labels are a permutation of 0..n_vars-1;
 *   else one reason: bit 1 short row, bit 2 a label outside 0..n_vars-1 (a PACE label below 3 included), bit 3 repeated label.
 * labels / preds: the row codec of dvs_build_records, device u8 [batch][n_vars] and [batch][n_vars] u16 (u64 when
 *   preds_are_u64), byte-identical to the host's encode_graphs of the decoded graph on valid rows.
 * keys: device u64 [batch][n_vars] (keys_bytes >= batch * n_vars * 8), the structure in data-set variable indices:
 *   bit label[u] of keys[b][label[v]] <=> edge u -> v, i.e. what dvs_bic_parent_masks makes of the codec — ready for
 *   dvs_bic_scores — and in bijection with the Bayesian-network structure whatever vertex order the decoder grew.
 * hashes: device u64 [batch]: a fixed mixing function of the key words in variable order, & hash_mask & (2^63 - 1)
 *   (pass all ones in production; a small mask forces collisions for tests).  63 bits: signed and unsigned sorts agree.
 * Invalid rows get zero labels / preds / keys and the hash DVS_STRUCT_HASH_INVALID, which sorts last.
 * 1 <= n_vars <= 45; batch <= 2^30.  (Added in ABI 202 as a pure addition: the version number stays.) */
#define DVS_STRUCT_HASH_INVALID 0x7fffffffffffffffull
int dvs_decoded_structures(int32_t batch, int32_t n_vars, int32_t preds_are_u64, const void* states, size_t state_bytes,
                           uint64_t hash_mask, uint8_t* flags, uint8_t* labels, void* preds, uint64_t* keys,
                           size_t keys_bytes, uint64_t* hashes, void* stream);

/* Exact, deterministic "new structure" filter of such a batch against a device-resident set of structures already seen
 * (the `seen` set of search.new_structures).  sorted_hashes: device u64 [batch], the batch's hashes in ascending order;
 * order: device i64 [batch], the row index of every sorted position, from a STABLE sort (equal hashes keep row order);
 * keys (keys_bytes >= batch * n_vars * 8) / flags: as dvs_decoded_structures wrote them, in row order.  The set: seen_hashes
 * device u64 [seen_count] ascending, seen_keys device u64 [seen_count][n_vars] (seen_keys_bytes >= seen_count * n_vars * 8);
 * both may be NULL when seen_count == 0.  out: device u8 [batch] in row order: 1 new (bit 0 of flags set, key not in the
 * set, no row of smaller index in the batch has the same key), 2 key in the set, 4 duplicate of an earlier row (not in the
 * set), 0 flags bit 0 clear.  Equality is decided on the full key, never on the hash: results do not depend on hash
 * collisions, only the time does (a row is compared with every different key of equal hash that sorts before it; equal
 * keys stop at the first).  No atomics: the output is a pure function of the inputs, two calls give equal bytes.
 * batch == 0 returns 0 and enqueues nothing.  (Added in ABI 202 as a pure addition: the version number stays.) */
int dvs_structset_filter(int32_t batch, int32_t n_vars, const uint64_t* sorted_hashes, const int64_t* order,
                         const uint64_t* keys, size_t keys_bytes, const uint8_t* flags, int32_t seen_count,
                         const uint64_t* seen_hashes, const uint64_t* seen_keys, size_t seen_keys_bytes, uint8_t* out,
                         void* stream);

/* Training graphs on the device: `batch` Erdos-Renyi DAGs (the reference's LabeledDag.generate_random_graph_erdos_renyi,
 * src/toolkit/labeled.py:281-333) written as the row codec of dvs_build_records, one launch, no host pass.
 * DAG b has n_vars vertices and m = num_edges[b] (device i32 [batch]) edges among the P = n_vars (n_vars - 1) / 2 slots;
 * slot t = v (v - 1) / 2 + u is the edge u -> v, u < v (igraph's Erdos_Renyi(n, m) + to_directed("acyclic"): a uniform
 * m-subset of the unordered pairs, oriented low -> high).  With the counter-based draws of the dropout masks
 * (key = site_key(seed, site, dag_offset + b), sites 300 edges / 301 labels), attempt a = 0, 1, .. takes slot t, in slot
 * order, iff (draw(key_e, a * 1024 + t) * (P - t)) >> 32 < m - (slots taken so far): selection sampling, exactly m edges.
 * The result is the first attempt in attempt order that is weakly connected over all vertices (over the vertices of degree
 * >= 1 with DVS_GEN_ACCEPT_ISOLATES; attempt 0 with DVS_GEN_ACCEPT_NO_CONNECTIVITY).  Labels, drawn once after acceptance:
 * without replacement ('sample', needs card >= n_vars: r = (draw(key_l, v) * (card - v)) >> 32, the r-th lowest unused
 * value) or, with DVS_GEN_LABELS_CHOICE, (draw(key_l, v) * card) >> 32.  Vertices are in generation order, which is
 * topological.  labels: device u8 [batch][n_vars]; preds: device [batch][n_vars], u16 for n_vars <= 13 and u64 above
 * (preds_are_u64 must say so), bit u of preds[b][v] <=> u -> v; attempts: device i32 [batch]: the 1-based accepted attempt,
 * 0 when none of try_limit was accepted, -1 when m is outside [n_vars - 1, P]; for 0 and -1 the DAG's rows are zero.
 * A pure function of (seed, dag_offset + b, m, n_vars, card, try_limit, flags & 7): two calls give equal bytes, a batch
 * split over calls or ranks by dag_offset gives the bytes of the whole batch, and the lane mapping does not matter.
 * Bits DVS_GEN_GROUP_SHIFT .. +3 of flags, tuning only: 0 lets the library choose how many lanes share a DAG (they try
 * consecutive attempts side by side, the lowest accepted one wins), k = 1 .. 7 asks for 2^(k-1).
 * 2 <= n_vars <= 45, 1 <= card <= 45, 1 <= try_limit <= 4096, batch <= 2^30; code 14 with the needed size for a short preds
 * buffer.  (Added in ABI 202 as a pure addition: the version number stays.) */
#define DVS_GEN_LABELS_CHOICE 1
#define DVS_GEN_ACCEPT_ISOLATES 2
#define DVS_GEN_ACCEPT_NO_CONNECTIVITY 4
#define DVS_GEN_GROUP_SHIFT 8
int dvs_generate_dags(int32_t batch, int32_t n_vars, int32_t card, int32_t preds_are_u64, const int32_t* num_edges,
                      uint64_t seed, int64_t dag_offset, int32_t try_limit, int32_t flags, uint8_t* labels, void* preds,
                      size_t preds_bytes, int32_t* attempts, void* stream);

/* Per-DAG edge counts for dvs_generate_dags, drawn on the device: DAG b gets edge_counts[i] (device i32 [n_entries]) with
 * probability weight_i / W, where cum_weights (device i32 [n_entries]) holds the running sums of the positive integer
 * weights and W = cum_weights[n_entries - 1] < 2^31: i is the first entry with cum_weights[i] > (draw(key_m, 0) * W) >> 32,
 * key_m = site_key(seed, 302, dag_offset + b).  num_edges: device i32 [batch].  The mixture of a shuffled curriculum data
 * set (schema entry i weighs (i + 1)^2), sharded by dag_offset like the graphs themselves.  1 <= n_entries <= 1024.
 * (Added in ABI 202 as a pure addition: the version number stays.) */
int dvs_generate_edge_counts(int32_t batch, int32_t n_entries, const int32_t* edge_counts, const int32_t* cum_weights,
                             uint64_t seed, int64_t dag_offset, int32_t* num_edges, void* stream);

/* BIC of B discrete Bayesian-network structures on one data set (replaces BNLearnWrapper.score,
 * src/problem/bn/bnlearn.py:27-61 = `Rscript bnlearn_score.R`: bnlearn::score(net, data, type = "bic")).
 * data: device u64 [n_samples][ceil(n_vars/16)], variable i's level code (0..15) in bits 4*(i%16).. of word i/16;
 * card: device u8 [n_vars] level counts; parents: device u64 [B][n_vars], bit u of parents[b][v] <=> edge u -> v in
 * DATASET variable indices (bnlearn.py:40-45 maps graph vertex v to variable labels[v]); scratch: device f64
 * [B][n_vars]; out: device f64 [B].  Tables of up to 36 864 (configuration, level) cells are counted densely in LDS;
 * larger parent sets go through an LDS sort of the samples, which needs n_samples <= 16 384 and <= 63 key bits —
 * otherwise bit 4 of status (device int32, zeroed by the caller) is set and that DAG's score is NaN.  n_vars <= 48. */
int dvs_bic_scores(int32_t batch, int32_t n_vars, int32_t n_samples, const uint64_t* data, const uint8_t* card,
                   const uint64_t* parents, double* scratch, double* out, int32_t* status, void* stream);

/* bnlearn's other decomposable discrete scores from the same counts (the reference passes metric_name straight to
 * bnlearn::score(net, data, type = metric_name), bnlearn_scripts/bnlearn_score.R; mirror: BNLearnWrapper(metric_name=...)).
 * Per variable, with N_jk the count of parent configuration j and level k, N_j = sum_k N_jk, r the variable's level count,
 * q the product of its parents' level counts and S = n_samples, the local score is
 *   DVS_SCORE_LOGLIK  sum N_jk log(N_jk / N_j)
 *   DVS_SCORE_AIC     loglik - k (r - 1) q                                  score_arg = k >= 0, default 1
 *   DVS_SCORE_BIC     loglik - k (r - 1) q                                  score_arg = k >= 0, default log(S) / 2
 *   DVS_SCORE_BDE     sum_j [ lgamma(a_j) - lgamma(a_j + N_j) + sum_k ( lgamma(a_jk + N_jk) - lgamma(a_jk) ) ]  (BDeu)
 *                     with a_jk = iss / (r q), a_j = iss / q                score_arg = iss > 0, default 1
 *   DVS_SCORE_BDS     as BDE with q replaced by the number of parent configurations observed in the data
 *   DVS_SCORE_K2      as BDE with a_jk = 1, a_j = r                         no argument
 *   DVS_SCORE_BDJ     as BDE with a_jk = 1/2, a_j = r / 2                   no argument
 * and the score of a structure is the sum over its variables (uniform graph prior: nothing added).  Empty cells and
 * unobserved configurations contribute exactly zero.  score_arg = NaN asks for the type's default and is the only value
 * the types without an argument take.  Everything else — buffers, limits, status bit 4, scratch = the local scores
 * [B][n_vars] — is dvs_bic_scores'; DVS_SCORE_BIC with NaN gives the bytes dvs_bic_scores gives.  Checked before anything
 * is enqueued: code 12 for a score_type that is not in the enum, 13 for a score_arg the type does not take (iss not
 * finite or <= 0, k negative or not finite, any number for a type without an argument).  fp64 throughout, fixed summation
 * order: two calls give equal bytes.  (Added in ABI 202 as a pure addition: the version number stays.) */
typedef enum dvs_score_type {
    DVS_SCORE_LOGLIK = 0,
    DVS_SCORE_AIC = 1,
    DVS_SCORE_BIC = 2,
    DVS_SCORE_BDE = 3,
    DVS_SCORE_BDS = 4,
    DVS_SCORE_K2 = 5,
    DVS_SCORE_BDJ = 6
} dvs_score_type;
int dvs_bn_scores(int32_t batch, int32_t n_vars, int32_t n_samples, const uint64_t* data, const uint8_t* card,
                  const uint64_t* parents, int32_t score_type, double score_arg, double* scratch, double* out,
                  int32_t* status, void* stream);

/* Greedy hill climbing over single-edge moves, step 1 of 2: the neighbourhood's local scores.
 *   toggles[b][v][u] (device f64 [B][n_vars][n_vars]) = the local score of variable v with parent set parents[b][v] xor
 *   (1 << u), u != v (the diagonal is NaN); local[b][v] (device f64 [B][n_vars]) = the local score as it stands.
 * One table prices every move on u -> v: add and delete are toggles[v][u] - local[v], a reversal is
 * (toggles[v][u] - local[v]) + (toggles[u][v] - local[u]).  Every cell is, bit for bit, what dvs_bn_scores writes into
 * scratch[.][v] for a row holding that parent set (same score_type / score_arg, data, card, limits); a refused family
 * (table too large for both counting paths, a parent bit >= n_vars) is NaN in its cell alone and sets status bit 4 — it
 * means "this move is not available", not an error.
 * worklist null: all B * n_vars rows.  worklist device i32 [2 * batch] (written by dvs_hc_step): slots 2b and 2b + 1 name
 * the rows of structure b to recompute, -1 = none; only those rows of toggles are written, local is left to dvs_hc_step.
 * Checked before anything is enqueued: codes 12 / 13 as dvs_bn_scores, 14 with the needed size for local_bytes <
 * batch * n_vars * 8 or toggles_bytes < batch * n_vars^2 * 8; batch * n_vars^2 < 2^31.  (Added in ABI 202 as a pure addition:
 * the version number stays.) */
int dvs_bn_toggle_scores(int32_t batch, int32_t n_vars, int32_t n_samples, const uint64_t* data, const uint8_t* card,
                         const uint64_t* parents, int32_t score_type, double score_arg, const int32_t* worklist,
                         double* local, size_t local_bytes, double* toggles, size_t toggles_bytes, int32_t* status,
                         void* stream);

/* Step 2 of 2: one greedy move per structure, in place.  With reach[v] the ancestors of v in parents[b]:
 *   add u -> v      u not in P[v], v not an ancestor of u, |P[v]| < max_parents, bit u not in forbidden[v]
 *   delete u -> v   u in P[v]
 *   reverse u -> v  u in P[v], no child of u other than v is v's ancestor, |P[u]| < max_parents, bit v not in forbidden[u]
 * and every toggles cell the move's delta reads is not NaN.  The move with the largest fp64 delta (expressions above, in
 * that operand order) wins, exact ties go to the lowest code = op * n_vars^2 + v * n_vars + u (op 0 add, 1 delete,
 * 2 reverse).  If delta > min_delta: parents' rows are updated, local[v] (and local[u]) are copied from toggles, the
 * changed rows go into worklist slots 2b, 2b + 1 (for dvs_bn_toggle_scores), steps[b] += 1 and, with trace (device i64
 * [batch][step_cap][2], nullable), (code, the delta's bits) is stored at trace[b][steps[b] before the move].  Otherwise
 * converged[b] = 1 and both slots are -1.  A structure with converged[b], flags[b] or steps[b] >= step_cap is left alone.
 * flags[b] (device i32, zeroed by the caller): bit 0 the structure has a cycle, bit 1 one of its local scores is NaN;
 * either freezes it at zero steps.  max_parents <= 0: no cap.  forbidden: device u64 [n_vars] shared by the batch, nullable.
 * steps, converged: device i32 [batch], zeroed by the caller before the first step.  *active (device i32, zeroed by the
 * caller) += the number of structures that moved in this call.  Nothing depends on the order in which structures are
 * processed: two runs give equal bytes.  Codes: 13 for a NaN min_delta or step_cap < 1, 14 with the needed size for
 * toggles_bytes < batch * n_vars^2 * 8 or trace_bytes < batch * step_cap * 16.  (Added in ABI 202 as a pure addition: the
 * version number stays.) */
int dvs_hc_step(int32_t batch, int32_t n_vars, uint64_t* parents, double* local, const double* toggles, size_t toggles_bytes,
                int32_t max_parents, double min_delta, const uint64_t* forbidden, int32_t step_cap, int32_t* worklist,
                int32_t* steps, int32_t* converged, int32_t* flags, int64_t* trace, size_t trace_bytes, int32_t* active,
                void* stream);

/* Tabu search over the same moves: one move per structure, in place, whatever its sign.  Arguments, move
 * codes, legality (the NaN-cell rule included), delta expressions, flags, worklist, steps, trace and *active are those of
 * dvs_hc_step; in addition, all device buffers:
 *   ring          u64 [batch][tabu_len][n_vars]: the structures recently stood on
 *   visited       i32 [batch], zeroed by the caller: structures pushed so far; the push slot is visited % tabu_len and the
 *                 valid entries are the first min(visited, tabu_len)
 *   stall         i32 [batch], zeroed by the caller: consecutive moves that did not raise the best
 *   best_score    f64 [batch], set to -inf by the caller; best_parents u64 [batch][n_vars]
 * A structure with converged[b], flags[b] or steps[b] >= step_cap is left alone: both worklist slots -1, nothing else
 * written.  A cycle or a NaN local score sets flags[b] as in dvs_hc_step and freezes the structure at zero steps, before
 * anything below.  Otherwise, with S(P) = local[0] + local[1] + ... + local[n_vars - 1] added left to right in fp64 (the
 * order in which dvs_bn_scores adds its total):
 *   1. first call (visited[b] == 0): best_score[b] = S(start), best_parents[b] = the start.
 *   2. push: the current structure is stored at slot visited[b] % tabu_len and visited[b] += 1.
 *   3. a move is tabu iff the structure it produces equals, row for row, one of the valid ring entries (the current
 *      structure is one of them).  Exact: no hashing.  Among the legal moves that are not tabu the largest fp64 delta wins,
 *      exact ties go to the lowest code; the move is taken whatever its sign.  If there is none: converged[b] = 1, both
 *      slots -1, the structure is not touched.
 *   4. apply, as dvs_hc_step: rows, local from toggles, worklist slots, steps[b] += 1, trace (code, delta bits), *active += 1.
 *   5. S' = S(new structure) from the updated local.  If S' - best_score[b] > min_delta (strict): best_score[b] = S',
 *      best_parents[b] = the new rows, stall[b] = 0.  Otherwise stall[b] += 1, and at stall[b] >= max_stall converged[b] = 1;
 *      the move stays applied and the worklist stays written, so the tables match parents after the toggle pass.
 * Nothing depends on the order in which structures are processed: two runs give equal bytes.  Codes: 13 for tabu_len < 1,
 * max_stall < 1, a NaN min_delta or step_cap < 1; 14 with the needed size for toggles_bytes, trace_bytes (as dvs_hc_step),
 * ring_bytes < batch * tabu_len * n_vars * 8 or best_bytes < batch * n_vars * 8.  (Added in ABI 202 as a pure addition: the
 * version number stays.) */
int dvs_tabu_step(int32_t batch, int32_t n_vars, uint64_t* parents, double* local, const double* toggles, size_t toggles_bytes,
                  int32_t max_parents, double min_delta, const uint64_t* forbidden, int32_t step_cap, int32_t* worklist,
                  int32_t* steps, int32_t* converged, int32_t* flags, int64_t* trace, size_t trace_bytes, int32_t* active,
                  int32_t tabu_len, uint64_t* ring, size_t ring_bytes, int32_t* visited, int32_t max_stall, int32_t* stall,
                  double* best_score, uint64_t* best_parents, size_t best_bytes, void* stream);

/* One uniformly random legal move per structure, in place (the perturbation of a random restart).  Legality is that of
 * dvs_hc_step, "every toggles cell the move's delta reads is not NaN" included, so local can be copied from toggles; the
 * scores are not looked at otherwise.  With M legal moves in ascending code order the move taken is number
 * (uint64(r) * M) >> 32, r = dvs_draw(dvs_site_key(seed_lo, seed_hi, 400, b), draw_index) of csrc/dvs_device.h (b the
 * structure's index in the batch; oracle/rng.py restates both functions); move k is taken with probability within 2^-32 of
 * 1 / M, a bias of at most M / 2^32 in all.  The rows, local and the worklist slots are written as by a step, so the
 * incremental dvs_bn_toggle_scores pass follows; steps, trace and converged do not exist here.  M = 0, or flags[b] set on entry or
 * by this call (cycle, NaN local score, as dvs_hc_step): the structure is untouched and both slots are -1.  Code 14 with the
 * needed size for toggles_bytes < batch * n_vars^2 * 8.  (Added in ABI 202 as a pure addition: the version number stays.) */
int dvs_hc_perturb(int32_t batch, int32_t n_vars, uint64_t* parents, double* local, const double* toggles, size_t toggles_bytes,
                   int32_t max_parents, const uint64_t* forbidden, int32_t* worklist, int32_t* flags, uint64_t seed,
                   uint32_t draw_index, void* stream);

/* Structure comparison.  A PDAG is stored like a parent-mask batch, device u64 [B][n_vars]: bit u of row v is
 * set iff u -> v or u - v; an undirected edge u - v has bit u of row v and bit v of row u, a directed one u -> v only bit u of
 * row v (bnlearn's amat).  A DAG's parent masks are a PDAG in this form.
 *
 * dvs_cpdag: parents (device u64 [batch][n_vars], any variable order) -> pdag (device u64 [batch][n_vars]), the completed
 * PDAG of each DAG's Markov equivalence class: the skeleton, the v-structures (u -> v is compelled if v has a parent that is
 * neither u nor adjacent to u), then Meek's rules to a fixpoint, each for an undirected u - v, with all orientations of a
 * round found first and applied together:
 *   R1  u -> v if some w -> u is not adjacent to v
 *   R2  u -> v if u -> w -> v for some w
 *   R3  u -> v if u - w1 -> v and u - w2 -> v for two non-adjacent w1, w2
 * (R4 cannot fire when the start is a DAG's own v-structures.)  An edge is directed in pdag iff it has that direction in
 * every DAG of the class.  flags (device i32 [batch], written for every structure): 0, or 2 = a parent bit >= n_vars or a
 * self-loop, or else 1 = the rows have a directed cycle; a flagged structure gets all-zero pdag rows and does not affect the
 * others.  Integers only: two runs give equal bytes.  Checked before anything is enqueued, in this order: batch > 0 (2),
 * n_vars in [1, 48] (3), batch * n_vars < 2^31 (2), null pointers (10), pdag_bytes < batch * n_vars * 8 (14 with the needed
 * size).  (Added in ABI 202 as a pure addition: the version number stays.) */
int dvs_cpdag(int32_t batch, int32_t n_vars, const uint64_t* parents, uint64_t* pdag, size_t pdag_bytes, int32_t* flags,
              void* stream);

/* Counts over the unordered pairs {u, v}, u != v, of two PDAG batches: a (device u64 [batch][n_vars], the learned side)
 * against b (device u64 [b_rows][n_vars], the target; b_rows = 1: one target for the whole batch, else b_rows = batch).  The
 * state of a pair in a mask is none, u -> v, v -> u or undirected; a pair is present when its state is not none.  Bits >=
 * n_vars and the diagonal of either side are ignored.  counts (device i32 [batch][5]):
 *   [0] shd      pairs whose states differ
 *   [1] tp       pairs present in a with the same state in b
 *   [2] fp       pairs present in a whose state differs in b
 *   [3] fn       pairs present in b whose state differs in a
 *   [4] hamming  pairs present in exactly one of the two
 * so a reversed arc, or a directed against an undirected edge, is shd 1, fp 1, fn 1; tp + fp is the number of edges of a and
 * tp + fn that of b.  On two outputs of dvs_cpdag, shd is the structural Hamming distance of Tsamardinos et al. (2006); on
 * DAG masks as they are, the counts are those of the DAGs.  Checked before anything is enqueued, in this order: batch > 0
 * (2), n_vars in [1, 48] (3), batch * n_vars < 2^31 (2), null pointers (10), b_rows not 1 or batch (12), counts_bytes <
 * batch * 20 (14 with the needed size).  (Added in ABI 202 as a pure addition: the version number stays.) */
int dvs_pdag_compare(int32_t batch, int32_t n_vars, const uint64_t* a, const uint64_t* b, int32_t b_rows, int32_t* counts,
                     size_t counts_bytes, void* stream);

/* Constraint-based structure learning: bnlearn's ci.test and pc.stable for discrete data.
 *
 * dvs_ci_tests: n_tests conditional-independence tests on one data set.  data, card, n_vars <= 48, n_samples as for
 * dvs_bn_scores; pairs (device i32 [n_tests][2]) names x and y of test t, cond (device u64 [n_tests]) its conditioning set Z as
 * a bit mask; out (device f64 [n_tests][3]) gets (statistic, df, p-value).  With n the counts over the samples of the
 * (z, x, y) table, n_xz, n_yz, n_z its marginals, r the level counts of card, sums over occupied cells, natural logarithms:
 *   DVS_CI_MI       statistic G^2 = 2 sum n_xyz log(n_xyz n_z / (n_xz n_yz));       df = (r_x - 1)(r_y - 1) prod r_z
 *   DVS_CI_X2       statistic X^2 = sum (n_xyz - e)^2 / e, e = n_xz n_yz / n_z, over the cells with e > 0;   df as MI
 *   DVS_CI_MI_ADF, DVS_CI_X2_ADF    the same statistics with df = sum_z max(rows_z - 1, 0) max(cols_z - 1, 0), rows_z (cols_z)
 *                   the number of x (y) levels with a non-zero marginal in configuration z; configurations with n_z = 0 add 0
 * The statistic is clamped at 0 (and written so); p = Q(df / 2, statistic / 2), the regularised upper incomplete gamma function
 * (its series below a + 1, a Lentz continued fraction above), and p = 1 for df = 0.  A test is refused — three NaNs and bit 4
 * of status (device int32, zeroed by the caller) — when r_x r_y prod r_z > max_cells, x = y, x or y is a member of Z, or any
 * index is < 0 or >= n_vars.  max_cells in [1, 36 864] also sizes the launch's LDS (max_cells * 4 bytes): pass the largest
 * table of the batch, not the limit.  Integer counts, fp64 arithmetic, fixed summation order: two calls give equal bytes.
 * Checked before anything is enqueued, in this order: n_tests, n_samples > 0 (2), n_vars in [1, 48] (3), test_type (12),
 * max_cells (13), null pointers (10), out_bytes < n_tests * 24 (14 with the needed size).  Parity with bnlearn's ci.test is
 * unpinned: the result rests on these definitions.  (Added in ABI 202 as a pure addition: the version number stays.) */
typedef enum dvs_ci_type {
    DVS_CI_MI = 0,
    DVS_CI_X2 = 1,
    DVS_CI_MI_ADF = 2,
    DVS_CI_X2_ADF = 3
} dvs_ci_type;
int dvs_ci_tests(int32_t n_tests, int32_t n_vars, int32_t n_samples, const uint64_t* data, const uint8_t* card,
                 const int32_t* pairs, const uint64_t* cond, int32_t test_type, int32_t max_cells, double* out,
                 size_t out_bytes, int32_t* status, void* stream);

/* One level of the PC-stable skeleton search, in two calls around dvs_ci_tests.  adj (device u64 [n_vars]) holds the adjacency
 * rows frozen at the start of the level; pair_xy (device i32 [n_pairs][2]) lists adjacent pairs x < y and offsets (device i64
 * [n_pairs + 1], offsets[0] = 0, offsets[n_pairs] = n_tests) where each pair's tests start (a pair may have none).  The tests of
 * a pair at level l are, in this order: the l-subsets of adj[x] \ {y} in ascending numeric order of their masks, then the
 * l-subsets of adj[y] \ {x} in the same order; a side with fewer than l members has none, and level 0 has the single empty
 * set.  dvs_pc_expand writes test t's (x, y) into pairs (device i32 [n_tests][2]) and its set into cond (device u64 [n_tests]),
 * each buffer tests_bytes >= n_tests * 8 bytes; a t that the offsets place outside its pair's tests gets (-1, -1), which
 * dvs_ci_tests refuses.  Checked in this order: n_pairs in [1, 1128] (2), n_vars in [1, 48] (3), n_tests in [1, 2^31 - 1] (2),
 * level in [0, 46] (13), null pointers (10), tests_bytes (14 with the needed size).
 *
 * dvs_pc_reduce reads cond and out (device f64 [n_tests][3], dvs_ci_tests' output over the whole level).  Pair p is separated
 * when some test of it has p-value > alpha; a NaN (refused) test never separates.  result (device i64 [n_pairs][2]) gets the
 * index of the lowest such test, or -1, and the pair's number of NaN tests.  For a separated pair sepset[x][y] = sepset[y][x]
 * = that test's cond (sepset: device u64 [n_vars][n_vars]; other cells are left as they are) and both adjacency bits are
 * clear in adj_next (device u64 [n_vars], written whole; may not alias adj); *refused (device i32, written) is the level's
 * NaN tests.  Checked in this order: n_pairs, n_vars, n_tests as above, alpha in [0, 1] (13), null pointers (10), sepset_bytes
 * < n_vars^2 * 8, then result_bytes < n_pairs * 16 (14 with the needed size).  Integers and comparisons only: two runs give
 * equal bytes.  (Added in ABI 202 as pure additions: the version number stays.) */
int dvs_pc_expand(int32_t n_pairs, int32_t n_vars, int32_t level, const uint64_t* adj, const int32_t* pair_xy,
                  const int64_t* offsets, int64_t n_tests, int32_t* pairs, uint64_t* cond, size_t tests_bytes, void* stream);
int dvs_pc_reduce(int32_t n_pairs, int32_t n_vars, const int32_t* pair_xy, const int64_t* offsets, int64_t n_tests,
                  const uint64_t* cond, const double* out, double alpha, const uint64_t* adj, uint64_t* adj_next,
                  uint64_t* sepset, size_t sepset_bytes, int64_t* result, size_t result_bytes, int32_t* refused, void* stream);

/* PC's orientation step on a batch: skeleton (device u64 [batch][n_vars], symmetric adjacency rows) and sepsets (device u64
 * [batch][n_vars][n_vars]) -> pdag (device u64 [batch][n_vars]) in the layout dvs_cpdag writes.  For every unshielded triple
 * x - z - y (x, y not adjacent) with z not in sepset[x][y], x -> z and y -> z are claimed; an edge claimed in both directions
 * stays undirected and is counted once in conflicts (device i32 [batch]).  Then Meek's rules R1 - R3 to a fixpoint exactly as
 * dvs_cpdag applies them.  flags (device i32 [batch]): 2 = illegal rows (an asymmetric skeleton, a bit >= n_vars, a self-loop;
 * pdag rows zero, conflicts 0), else 1 = the directed part of the result has a cycle (the rows are kept), else 0.  Checked in
 * this order: batch > 0 (2), n_vars in [1, 48] (3), batch * n_vars^2 < 2^31 (2), null pointers (10), sepsets_bytes < batch *
 * n_vars^2 * 8, then pdag_bytes < batch * n_vars * 8 (14 with the needed size).  Integers only: two runs give equal bytes.
 * (Added in ABI 202 as a pure addition: the version number stays.) */
int dvs_pc_orient(int32_t batch, int32_t n_vars, const uint64_t* skeleton, const uint64_t* sepsets, size_t sepsets_bytes,
                  uint64_t* pdag, size_t pdag_bytes, int32_t* conflicts, int32_t* flags, void* stream);

/* Parameters of a discrete Bayesian network: bnlearn's bn.fit, rbn and logLik(fitted, newdata) on the device.
 *
 * Layout of the conditional probability tables, shared by the three calls.  For variable v of structure b, r is its level count
 * card[v], q the product of its parents' level counts (1 without parents) and key the mixed-radix parent configuration with
 * the lowest variable id fastest: key = sum_i level(p_i) * prod_{i' < i} card[p_i'] over the parents p_0 < p_1 < ... (the
 * histogram index of dvs_bn_scores).  theta(v, key, k) = P(v = k | configuration key) is
 *   cpt[offsets[b * n_vars + v] + key * r + k]                                   (device f64)
 * with offsets device i64 [batch * n_vars + 1], non-decreasing, offsets[i + 1] - offsets[i] == q * r for every family i.  The
 * self bit of a parent row is ignored, as in dvs_bn_scores.  A family is malformed when a parent bit is >= n_vars, card[v] is
 * 0 or its slot in offsets does not have q * r cells.
 *
 * dvs_bn_fit: the tables of batch structures from one data set (data, card, n_vars <= 48, n_samples as for dvs_bn_scores).
 * With N_jk the count of configuration j and level k and N_j = sum_k N_jk:
 *   DVS_FIT_MLE    theta = N_jk / N_j, one fp64 division.  An unobserved configuration (N_j = 0) gets NaN in every cell with
 *                  unobserved = 0 (bnlearn's default) and 1 / r with unobserved = 1 (replace.unidentifiable = TRUE).
 *   DVS_FIT_BAYES  theta = (N_jk + a) / (N_j + r * a), a = iss / (r * q): bnlearn's method = "bayes".  fp64, the operations
 *                  in exactly that order and none fused; iss finite and > 0 (ignored by DVS_FIT_MLE, as unobserved is here).
 * A family is refused — its cells left unwritten, bit 4 of status (device int32, zeroed by the caller) set, the other
 * families of the launch written as usual — when it is malformed, when its slot ends beyond cpt_bytes, or when q * r > 36 864:
 * the counts live in the dense LDS table of dvs_bn_scores and no sorted-samples path exists here.  A data level >= card[v]
 * is not counted.  Integer counts, one rounding per operation: two calls give equal bytes.  Checked before anything is
 * enqueued, in this order: batch, n_samples > 0 (2), n_vars in [1, 48] (3), batch * n_vars < 2^31 (2), method (12), iss (13),
 * unobserved not 0 or 1 (12), null pointers (10), cpt_bytes < batch * n_vars * 8 (14 with that size: every family has a cell;
 * the slots themselves are device data and are checked there).
 *
 * dvs_bn_sample: n_rows rows drawn from ONE network by forward sampling: card, parents (device u64 [n_vars]) and offsets
 * (device i64 [n_vars + 1]) are those of the network — for structure b of a fitted batch pass parents + b * n_vars and
 * offsets + b * n_vars with the same cpt.  n_cells = offsets[n_vars] - offsets[0], which the caller knows from building
 * offsets.  data_out (device u64 [n_rows][ceil(n_vars / 16)]) gets the rows in the layout dvs_bic_scores reads, every word
 * written.  workspace: dvs_bn_sample_workspace_bytes(n_cells, n_vars) bytes of device memory (0 and dvs_last_error for
 * arguments out of range).  Two launches:
 *   prep   a topological order of parents (the lowest variable whose parents are all placed, repeatedly); u32 thresholds for
 *          every row (v, key) of the tables: with c_k = theta_0 + ... + theta_k added sequentially in fp64,
 *          T_k = min(floor(c_k * 2^31), 2^31), and T_k = 2^31 for every k at or beyond the last level with theta > 0.
 *          Status bits, each of which leaves data_out untouched: bit 0 a cycle; bit 4 a malformed
 *          family, card[v] > 16 or offsets[n_vars] - offsets[0] != n_cells; bit 6 a cell that is not finite or is negative, or a
 *          row with |c_{r-1} - 1| > 1e-9.
 *   draw   row i has the global index g = (row_offset + i) mod 2^32 and key = dvs_site_key(seed_lo, seed_hi, 500, g) of
 *          csrc/dvs_device.h (oracle/rng.py restates it).  Variable v draws h = dvs_draw(key, v); its level is the number of
 *          k < r - 1 with (h >> 1) >= T_k, its parents' levels being known by then.
 * So a level with theta = 0 is never drawn (a cumulative sum that has reached its last positive level has T = 2^31, above
 * every 31-bit draw, and a level of probability zero adds nothing to the count below it), and the bytes depend on (seed, g,
 * v) and the tables only: not on the order chosen, the launch geometry, whether the thresholds were staged in LDS (tables of
 * up to 8192 cells) or read from memory, or how a request is cut into calls with consecutive row_offset.  P(level = k) is
 * theta_k to within 2^-31 absolute.  Checked before anything is enqueued, in this order: n_rows in [1, 2^31 - 1] (2), n_vars
 * in [1, 48] (3), n_cells in [n_vars, 2^31 - 1] (2), row_offset >= 0 (12), null pointers (10), workspace_bytes (14 with the
 * needed size).
 *
 * dvs_bn_loglik: the log-likelihood of n_rows rows (data: device u64 [n_rows][ceil(n_vars / 16)], any rows, not the fit's)
 * under each of batch networks.  The term of a row is sum_v log theta(v, key_v, x_v), natural logarithm, added in ascending
 * v in fp64 starting from +0; per_row (device f64 [batch][n_rows], nullable) gets it.  out[b] (device f64 [batch]) is the sum
 * of the row terms in this order: rows 256 c .. 256 c + 255 (absent rows count +0) are added by the tree x[i] += x[i + s] for
 * s = 128, 64, ..., 1 over 256 slots; slot t of a second such array then adds the chunk sums c = t, t + 256, t + 512, ... in ascending c
 * starting from +0, and the same tree over those 256 slots gives out[b].  No floating-point atomics:
 * two calls give equal bytes, and per_row given or null gives the same out.  Nothing is special-cased: a row that meets
 * theta = 0 contributes -inf and one that meets NaN (or a negative cell) NaN, by IEEE arithmetic.  log theta is taken once per
 * cell into the workspace.  A malformed family, or a table that does not fit the workspace, makes out[b] and every row term of
 * that structure NaN and sets bit 4 of status; a row with a level >= card[v] for some v gets a NaN term (so out[b] is NaN) and
 * sets bit 4 too.  workspace (device): with chunks = ceil(n_rows / 256) and each array starting at the next multiple of 256
 * bytes: f64 [batch][chunks], i32 [batch][n_vars], then f64 [offsets[batch * n_vars] - offsets[0]].  Checked before anything is
 * enqueued, in this order: batch > 0 (2), n_rows in [1, 2^31 - 1] (2), n_vars in [1, 48] (3), batch * n_vars and batch * chunks
 * < 2^31 (2), null pointers (10; per_row may be null), workspace_bytes below the first two arrays plus batch * n_vars * 8 (14
 * with that size; the tables' own size is device data and is checked there).
 *
 * Parity with bnlearn's bn.fit, rbn, logLik and bn.cv is unpinned against an R run: the results rest on these definitions.
 * (Added in ABI 202 as pure additions: the version number stays.) */
typedef enum dvs_fit_method {
    DVS_FIT_MLE = 0,
    DVS_FIT_BAYES = 1
} dvs_fit_method;
int dvs_bn_fit(int32_t batch, int32_t n_vars, int32_t n_samples, const uint64_t* data, const uint8_t* card,
               const uint64_t* parents, int32_t method, double iss, int32_t unobserved, const int64_t* offsets, double* cpt,
               size_t cpt_bytes, int32_t* status, void* stream);
size_t dvs_bn_sample_workspace_bytes(int64_t n_cells, int32_t n_vars);
int dvs_bn_sample(int32_t n_vars, int64_t n_rows, const uint8_t* card, const uint64_t* parents, const int64_t* offsets,
                  const double* cpt, int64_t n_cells, uint64_t seed, int64_t row_offset, void* workspace, size_t workspace_bytes,
                  uint64_t* data_out, int32_t* status, void* stream);
int dvs_bn_loglik(int32_t batch, int32_t n_vars, int64_t n_rows, const uint64_t* data, const uint8_t* card,
                  const uint64_t* parents, const int64_t* offsets, const double* cpt, double* per_row, double* out,
                  void* workspace, size_t workspace_bytes, int32_t* status, void* stream);

/* Inference on a fitted network: bnlearn's cpquery, cpdist and predict on the device.  The CPT layout is the
 * one above.
 *
 * dvs_bn_lw: likelihood weighting on ONE network (card, parents, offsets, cpt, n_cells as for dvs_bn_sample), n_queries (Q)
 * queries of n_particles (M) particles each.  evidence: device u64 [Q][ceil(n_vars / 16)], rows in the layout of
 * dvs_bic_scores; observed: device u64 [Q], bit v set <=> variable v of query q is clamped to its level in evidence[q] (the
 * other nibbles of the row are not read); event: device u16 [n_vars], nullable: bit k of event[v] set <=> level k of v is
 * allowed, and a particle satisfies the event when the level of every variable is allowed (a conjunction of level sets); null
 * allows everything.  targets: a mask of the variables whose weighted marginals are wanted.  The preparation is that of
 * dvs_bn_sample (order, thresholds T_k, status bits 0 / 4 / 6, each of which leaves every output untouched).  Query q has the
 * global index g = (query_offset + q) mod 2^32 and key = dvs_site_key(seed_lo, seed_hi, 501, g).  Particle p of query q
 * starts with the weight w = 1.0 and takes the variables in the preparation's order:
 *   unobserved v   draws h = dvs_draw(dvs_draw(key, v), p); its level is the number of k < r - 1 with (h >> 1) >= T_k, as
 *                  in dvs_bn_sample.
 *   observed v     takes its evidence level x and w = w * theta, theta the cell of level x under the parent configuration of v
 *                  (the CPT layout above; the parents' levels are known by then), one fp64 multiplication; theta = 0 gives
 *                  exactly 0.
 * The particle index enters the last mixing step, next to the variable's: for a fixed (query, variable) p -> h is a bijection
 * of the 32-bit words, so two particles of one query never share a draw of any variable, however many there are — a derived
 * 32-bit per-particle key would make about M^2 / 2^33 pairs of particles of one query share all of theirs.
 * Outputs (device f64), cell by cell the sum over the particles of one value per particle:
 *   sums [Q][3]            w, w * w, and w if the particle satisfies the event else +0 (so [2] equals [0] for event null)
 *   marginals [Q][T][16]   given exactly when targets != 0; T = popcount(targets), targets in ascending id; cell k: w if the
 *                          target's level is k else +0; cells k >= card are +0.
 *   particles u64 [Q][M][ceil(n_vars / 16)], particle_weights f64 [Q][M]   both null or both given: bnlearn's cpdist.
 * Every sum is taken in this order, the one of dvs_bn_loglik: particles 256 c .. 256 c + 255 (absent ones count +0) are added
 * by the tree x[i] += x[i + s] for s = 128, 64, ..., 1 over 256 slots; slot t of a second such array then adds the chunk sums
 * c = t, t + 256, ... in ascending c starting from +0, and the same tree over those 256 slots gives the cell.  It does not
 * depend on the launch geometry, on whether the thresholds were staged in LDS, on which optional outputs are requested or on
 * how the queries are cut into calls with consecutive query_offset.  No floating-point atomics: two calls give equal bytes.
 * Status: a query with an observed bit >= n_vars or an evidence level >= card[v] sets bit 4 and gets NaN in every cell of
 * sums, marginals and particle_weights (its particle rows are zero words); the other queries are written as usual.  A query
 * whose weights sum to 0 (evidence of probability zero) is no error: its sums are plain zeros and bit 7 is set as
 * information.  workspace: dvs_bn_lw_workspace_bytes bytes (0 and dvs_last_error for arguments out of range).  Checked before
 * anything is enqueued, in this order: n_queries, n_particles in [1, 2^31 - 1] (2), n_vars in [1, 48] (3), n_cells in [n_vars,
 * 2^31 - 1] (2), n_queries * ceil(n_particles / 256) < 2^31 (2), a targets bit >= n_vars (12), query_offset >= 0 (12), null
 * pointers (10; event, marginals, particles and particle_weights may be null), marginals given exactly when targets != 0 (12),
 * particles and particle_weights both or neither (12), workspace_bytes (14 with the needed size).
 *
 * dvs_bn_blanket_posterior: the posterior of variable `target` given all the others, for n_rows rows (data as for
 * dvs_bn_loglik; the target's own column is ignored) under each of batch networks.  For level k of the target
 *   use_children = 0   p_k = theta_t(k | pa_t): bnlearn's predict(method = "parents");
 *   use_children = 1   p_k = theta_t(k | pa_t) * prod_c theta_c(x_c | pa_c with target = k), the children c of the target in
 *                      ascending id, one fp64 multiplication each in that order: the exact posterior, which
 *                      predict(method = "bayes-lw") with every other variable observed approximates.
 * posterior (device f64 [batch][n_rows][card[target]], nullable) gets p_k / (p_0 + p_1 + ... added in ascending k starting
 * from +0), one division per cell.  Up to 48 factors can underflow for extreme tables; a row whose products are all zero
 * gives NaN (0 / 0), as does one that meets a NaN cell.  pred (device u8 [batch][n_rows]) is the lowest level among the
 * largest posterior cells — bnlearn breaks such ties at random — and 255 for a row with a NaN cell.  A malformed family
 * (as for dvs_bn_loglik; also card[v] > 16 or a slot that ends beyond cpt_bytes) makes every row of that structure NaN / 255
 * and sets bit 4 of status; a row with a level >= card[v] for some v other than the target gets NaN / 255 and sets bit 4 too.
 * Checked before anything is enqueued, in this order: batch > 0 (2), n_rows in [1, 2^31 - 1] (2), n_vars in [1, 48] (3),
 * batch * n_vars and batch * ceil(n_rows / 256) < 2^31 (2), target in [0, n_vars) (12), use_children 0 or 1 (12), null
 * pointers (10; posterior may be null), cpt_bytes < batch * n_vars * 8 (14 with that size).
 *
 * Parity with bnlearn's cpquery, cpdist, predict and bn.cv(loss = "pred" / "pred-lw") is unpinned against an R run: the
 * results rest on these definitions.  (Added in ABI 202 as pure additions: the version number stays.) */
size_t dvs_bn_lw_workspace_bytes(int64_t n_cells, int32_t n_vars, int64_t n_queries, int64_t n_particles, uint64_t targets);
int dvs_bn_lw(int32_t n_vars, int64_t n_queries, int64_t n_particles, const uint8_t* card, const uint64_t* parents,
              const int64_t* offsets, const double* cpt, int64_t n_cells, const uint64_t* evidence, const uint64_t* observed,
              const uint16_t* event, uint64_t targets, uint64_t seed, int64_t query_offset, void* workspace,
              size_t workspace_bytes, double* sums, double* marginals, uint64_t* particles, double* particle_weights,
              int32_t* status, void* stream);
int dvs_bn_blanket_posterior(int32_t batch, int32_t n_vars, int64_t n_rows, const uint64_t* data, const uint8_t* card,
                             const uint64_t* parents, const int64_t* offsets, const double* cpt, size_t cpt_bytes,
                             int32_t target, int32_t use_children, double* posterior, uint8_t* pred, int32_t* status,
                             void* stream);
/* Exact inference by variable elimination is declared in the companion header dvs_eliminate.h, which includes this one. */

/* Exact structure search: the DAG with the largest decomposable score, by the subset dynamic programme of
 * Silander and Myllymaki (2006).  table (device f64 [batch][2^n_vars][n_vars]): cell [t][S][v] is the local score of
 * variable v with parent set S & ~(1 << v) — what dvs_bn_scores writes into scratch for a batch whose row S holds
 * parents[v] = S & ~(1 << v); a NaN cell means "this family is not available" (refused, or never scored).  The batch is
 * batch independent tables.  fp64 throughout, every result defined by a total order: two runs give equal bytes.
 *   admissible   P is admissible for v when bit v is not in P, popcount(P) <= max_parents (max_parents <= 0: no cap),
 *                P & forbidden[v] == 0 (forbidden: device u64 [n_vars], nullable, shared by the batch, as in dvs_hc_step)
 *                and table[P][v] is not NaN.
 *   best, arg    for every S and every v not in S: best[S][v] is the largest table[P][v] over the admissible P that are
 *                subsets of S and arg[S][v] (u32) that P; exact fp64 ties go to the numerically smallest P.  No admissible P
 *                (only when table[0][v] is NaN): best = -inf, arg = 0xFFFFFFFF.  Cells with v in S are unspecified.
 *   R, sink      R[0] = +0.0 (sink[0] = -1).  For non-empty W: R[W] is the largest R[W ^ (1 << s)] + best[W ^ (1 << s)][s]
 *                over s in W, the operands in that order, one fp64 addition; sink[W] (i32) is that s, ties to the lowest s.
 *   backtrack    W = all ones; for k = n_vars - 1 down to 0: s = sink[W], order[k] = s, parents[s] = arg[W ^ (1 << s)][s],
 *                W ^= 1 << s.  score = R[all ones].  score == -inf: flags[t] = 1, parents all zero, order all -1; otherwise
 *                flags[t] = 0.  order is a topological order: parents[order[k]] has bits only among order[0 .. k-1].
 * Outputs: parents u64 [batch][n_vars] (bit u of parents[v] <=> u -> v), order i32 [batch][n_vars], score f64 [batch], flags
 * i32 [batch] (all written for every table).  workspace (dvs_exact_workspace_bytes bytes) holds the stages for callers and
 * tests to read, each array starting at the next multiple of 256 bytes: best f64 [batch][2^n_vars][n_vars], then arg u32
 * [batch][2^n_vars][n_vars], then R f64 [batch][2^n_vars], then sink i32 [batch][2^n_vars].  Checked before anything is
 * enqueued, in this order: batch > 0 (2), n_vars in [1, 20] (3), batch * 2^n_vars * n_vars < 2^31 (2), null pointers (10;
 * forbidden may be null), table_bytes < batch * 2^n_vars * n_vars * 8, then workspace_bytes < dvs_exact_workspace_bytes (14
 * with the needed size).  dvs_exact_workspace_bytes returns 0 (and sets dvs_last_error) when the first three fail.  Parity
 * with an external exact solver is unpinned: the result rests on these definitions and on brute force over all DAGs of up to
 * five vertices.  (Added in ABI 202 as a pure addition: the version number stays.) */
size_t dvs_exact_workspace_bytes(int32_t batch, int32_t n_vars);
int dvs_exact_search(int32_t batch, int32_t n_vars, const double* table, size_t table_bytes, int32_t max_parents,
                     const uint64_t* forbidden, void* workspace, size_t workspace_bytes, uint64_t* parents, int32_t* order,
                     double* score, int32_t* flags, void* stream);

/* Exact posterior arc probabilities: P(u -> v | data) summed over every DAG, by the subset dynamic programme
 * of Koivisto and Sood (2004) with the feature step of Koivisto (2006).  With bde or k2 local scores exp(cell) is a marginal
 * likelihood and the result is Bayesian model averaging; log_z is then the log marginal likelihood of the data under the
 * structure prior.  table, admissible, max_parents and forbidden are exactly those of dvs_exact_search.  size_prior (device
 * f64 [n_vars], nullable: all zeros): size_prior[k] is added to every admissible cell with popcount(P) = k.  f(v,P) is the
 * resulting value, -inf where P is not admissible for v.  Everything below is a natural log in fp64; lse is log-sum-exp, and
 * lse of nothing or of all -inf is -inf, never NaN.  V is the full set.
 *   alpha[S][v]   for v not in S: the lse of f(v,P) over the admissible P that are subsets of S.
 *   L[W]          L[0] = 0; for non-empty W the lse over v in W of alpha[W \ v][v] + L[W \ v].
 *   Rb[T]         Rb[0] = 0; for non-empty T the lse over v in T of alpha[V \ T][v] + Rb[T \ v] (v is the first of T to be
 *                 placed after V \ T).
 *   log_z         L[V]; log_z_back = Rb[V] is the same sum taken in the other order, a built-in cross-check.
 *   gamma[P][v]   for v not in P: the lse over all S that contain P and not v of L[S] + Rb[V \ S \ v] (-inf for v in P).
 *   family[P][v]  exp(f(v,P) + gamma[P][v] - log_z): the posterior probability that the parent set of v is exactly P; 0 where
 *                 P is not admissible.  Every exponent is <= 0 up to rounding: this one step is in the linear domain.
 *   prob[u][v]    the sum over the P that contain u of family[P][v] = P(u -> v | data); a forbidden arc is exactly 0.0.
 *   flags[t]      1 when log_z is -inf (no admissible DAG): prob and family are then all zero and no NaN appears anywhere;
 *                 otherwise 0.
 * Each cell of L and Rb is one max, one exp per term in ascending v and one log; alpha and gamma are folded bit by bit with
 * pairwise log-adds; the sums of prob have a fixed order: two runs give equal bytes.  Cells of alpha with v in S are
 * unspecified.
 * THE PRIOR IS ORDER-MODULAR, NOT UNIFORM OVER DAGS: it is uniform over the n! variable orders and, apart from size_prior,
 * uniform over the admissible parent sets within an order, so a DAG's prior weight is proportional to its number of linear
 * extensions (the empty graph counts n! times, a chain once).  This is the known bias of the method (Koivisto and Sood 2004,
 * Friedman and Koller 2003), kept deliberately: removing it costs 3^n.
 * Outputs: prob f64 [batch][n_vars][n_vars], log_z f64 [batch][2] (forward, backward), family f64 [batch][2^n_vars][n_vars]
 * (nullable: not stored), flags i32 [batch].  workspace (dvs_arc_posterior_workspace_bytes bytes) holds the stages for callers
 * and tests to read, each array starting at the next multiple of 256 bytes: gamma (alpha until the chains are done) f64
 * [batch][2^n_vars][n_vars], then L f64 [batch][2^n_vars], then Rb f64 [batch][2^n_vars], then the per-workgroup partial sums
 * of prob, f64 [batch][G][n_vars][n_vars] with rows = 256 / n_vars, sweeps = max(8, ceil(2^n_vars / (2048 rows))) and
 * G = ceil(2^n_vars / (rows sweeps)).  Checked before anything is enqueued, in this order and with the codes of
 * dvs_exact_search: batch > 0 (2), n_vars in [1, 20] (3), batch * 2^n_vars * n_vars < 2^31 (2), null pointers (10; forbidden,
 * size_prior and family may be null), table_bytes, workspace_bytes, then family_bytes when family is given (14 with the
 * needed size).  dvs_arc_posterior_workspace_bytes returns 0 (and sets dvs_last_error) when the first three fail.  Parity with
 * an external implementation is unpinned: the result rests on these definitions and on brute force over all DAGs of up to
 * five vertices.  (Added in ABI 202 as pure additions: the version number stays.) */
size_t dvs_arc_posterior_workspace_bytes(int32_t batch, int32_t n_vars);
int dvs_arc_posterior(int32_t batch, int32_t n_vars, const double* table, size_t table_bytes, int32_t max_parents,
                      const uint64_t* forbidden, const double* size_prior, void* workspace, size_t workspace_bytes,
                      double* prob, double* log_z, double* family, size_t family_bytes, int32_t* flags, void* stream);

/* Order MCMC: posterior arc probabilities and an order-space structure search for n_vars <= 48, by the
 * Metropolis sampler over variable orders of Friedman and Koller (2003).  Its stationary distribution is the order-modular
 * posterior of dvs_arc_posterior restricted to the families of the list, so for n_vars <= 20 that call is its exact yardstick.
 * THE PRIOR IS ORDER-MODULAR, NOT UNIFORM OVER DAGS (see dvs_arc_posterior): uniform over the n! orders and over the listed
 * parent sets within an order, so a DAG weighs in with its number of linear extensions.
 *
 * The family list replaces the 2^n table: offsets (device i64 [n_vars + 1]), sets (device u64 [n_families]), scores (device f64
 * [n_families]).  The families of v are the entries offsets[v] .. offsets[v + 1] - 1; offsets[0] = 0, offsets[n_vars] =
 * n_families, every variable has at least one entry and its entry 0 is the empty set; a mask of v holds neither bit v nor a
 * bit >= n_vars; scores are finite (f(v, P) of dvs_arc_posterior, the inadmissible sets left out).  These properties are
 * checked ON THE DEVICE by a first kernel; nothing is read back.  flags (device i32 [1]) is written: 0, or the bits 1 (offsets),
 * 2 (an entry 0 that is not the empty set), 4 (a mask bit), 8 (a score that is not finite), and the run is then skipped: every
 * other output stays untouched.  Bit 16: a chain whose `order` (init = 0) is not a permutation of 0 .. n_vars - 1; that chain
 * alone is skipped.
 *
 * Definitions (natural logs, fp64).  For a variable v and a set Q of variables, a family j of v is consistent with Q when
 * sets[j] & ~Q == 0.
 *   term(v, Q)    the log-sum-exp of scores[j] over the consistent families of v: never empty (entry 0).  Computed as
 *                 bestf + log(sum of exp(scores[j] - bestf)).
 *   bestf(v, Q)   the largest consistent score; arg(v, Q) its mask; exact ties go to the lower list index.
 *   pred(v)       the variables before v in the order; the score of an order is the sum over v of term(v, pred(v)), added
 *                 in ascending v.
 * Terms are always recomputed from the list, never updated incrementally: nothing drifts, and a cached term is the bytes a
 * fresh one would be.
 * Randomness.  Chain c has the global index g = (chain_offset + c) mod 2^32 and the key K = dvs_site_key(seed_lo, seed_hi, 700,
 * g) of csrc/dvs_device.h (oracle/rng.py restates dvs_site_key and dvs_draw).  init = 1: the start order is a Fisher-Yates
 * shuffle of the identity with the key K' of site 701: for k = n_vars - 1 down to 1, j = (uint64(dvs_draw(K', k)) * (k + 1))
 * >> 32, positions k and j are swapped.  init = 0: the caller's order.  Step s of the call is the global step t = step_offset
 * + s with the draws r0 = dvs_draw(K, 3 t), r1 = dvs_draw(K, 3 t + 1), r2 = dvs_draw(K, 3 t + 2):
 *   i = (r0 * (n_vars - 1)) >> 32,  m = min(window, n_vars - 1 - i),  j = i + 1 + ((r1 * m) >> 32)
 * and the proposal swaps the variables at positions i and j.  The probability of a pair of positions does not depend on the
 * state, so the proposal is symmetric.  Delta = S_new - S_old, each S the sum of the terms of the variables at positions
 * i .. j (of the proposed and of the current order) added in ascending position; one subtraction.  The proposal is accepted iff
 * log((r2 + 0.5) * 2^-32) < Delta.  n_vars = 1 proposes nothing.  A chain is a function of (seed, g, step index) only: a run
 * cut into calls with step_offset (order, accepted, sums, kept, best_score and best_parents handed on) or into shards with
 * chain_offset gives the bytes of the uncut run.
 * Kept samples.  After the accept decision of every global step t >= burn_in with (t - burn_in) % thin == 0:
 *   sums[c][u][v] += the sum over the consistent families j of v that contain u of exp(scores[j] - term(v, pred(v)))
 *                    = P(u -> v | order), the Rao-Blackwellised arc indicator;  kept[c] += 1.
 * Summation order (fixed: two runs give equal bytes).  Lane i of the chain's 256 takes a variable's families offsets[v] + i,
 * + 256, ... in that order, for the largest score, the sum of a term and the per-parent sums of a kept sample alike.  The 64
 * lanes of a wave meet in an xor butterfly (32, 16, ..., 1) for a term and are added in lane order for a kept sample; the four
 * waves are added in wave order.  No floating-point atomics.  The caller zeroes sums, kept and accepted and sets best_score to
 * -inf before the first call; later calls accumulate.
 * Best DAG seen.  At the start of a call and after every accepted move the order's best consistent DAG has the score sum over
 * v of bestf(v, pred(v)), added in ascending v; a strictly larger value replaces best_score[c], and arg(v, pred(v)) replaces
 * best_parents[c][v].
 * Outputs: order i32 [chains][n_vars] (in with init = 0, out always: position -> variable), log_score f64 [chains] (the final
 * order's score), accepted i32 [chains], sums f64 [chains][n_vars][n_vars], kept i32 [chains], best_score f64 [chains],
 * best_parents u64 [chains][n_vars], trace f64 [chains][steps] (nullable: the order's score after each step), flags i32 [1].
 *
 * dvs_order_mcmc_finish adds the chains' sums in a fixed tree (thread i adds chains i, i + 256, ... in that order, then the
 * tree of 128, 64, ..., 1) and kept as integers: prob[u][v] (device f64 [n_vars][n_vars]) = sum / kept, 0.0 when nothing was
 * kept.  The per-chain arrays stay for the between-chain spread.
 *
 * Checked before anything is enqueued, in this order: chains > 0, steps >= 0, n_families in [1, 2^31 - 1] (2), n_vars in
 * [1, 48] (3), chains * n_vars^2 < 2^31 (2), null pointers (10; trace may be null), chain_offset >= 0 and step_offset >= 0
 * (12), window in [1, max(1, n_vars - 1)], thin >= 1, burn_in >= 0, init in {0, 1}, 3 (step_offset + steps) < 2^32 (13), then
 * sets_bytes, scores_bytes, sums_bytes and, when trace is given, trace_bytes (14 with the needed size).
 * dvs_order_mcmc_finish: chains > 0 (2), n_vars (3), the product (2), null pointers (10), sums_bytes (14).  (Added in ABI 202
 * as pure additions: the version number stays.) */
int dvs_order_mcmc(int32_t chains, int32_t n_vars, int64_t n_families, int32_t steps, const int64_t* offsets,
                   const uint64_t* sets, size_t sets_bytes, const double* scores, size_t scores_bytes, uint64_t seed,
                   int64_t chain_offset, int64_t step_offset, int64_t burn_in, int32_t thin, int32_t window, int32_t init,
                   int32_t* order, double* log_score, int32_t* accepted, double* sums, size_t sums_bytes, int32_t* kept,
                   double* best_score, uint64_t* best_parents, double* trace, size_t trace_bytes, int32_t* flags, void* stream);
int dvs_order_mcmc_finish(int32_t chains, int32_t n_vars, const double* sums, size_t sums_bytes, const int32_t* kept,
                          double* prob, void* stream);

/* Model averaging: bnlearn's boot.strength, custom.strength, inclusion.threshold and averaged.network as
 * five building blocks.  All are pure additions to ABI 202: the version number stays.
 *
 * Row sets in the scorer.  dvs_bn_scores_rows and dvs_bn_toggle_scores_rows take the arguments of dvs_bn_scores and
 * dvs_bn_toggle_scores (the worklist included) and, after status, four more:
 *   rows      device i32 [n_sets][set_size], each entry in [0, n_samples)
 *   set_size, n_sets
 *   set_of    device i32 [batch], each in [0, n_sets); nullable: null means structure b uses set b (n_sets >= batch).
 * Structure b is scored on the data set of S = set_size samples whose sample i is data[rows[set_of[b]][i]].  Everything the
 * call writes for that structure — out, scratch, local, toggles, the NaN cells and status bit 4 — is, bit for bit, what the
 * plain entry point writes for it on that gathered data set: both counting paths are independent of the order of the
 * samples (integer atomics; sorted keys).  So bic's default k is log(set_size) / 2, the sorted-samples path holds
 * set_size <= 16 384, and set_size may be larger or smaller than n_samples.  PRECONDITION: the entries of rows and set_of
 * are NOT range-checked on the device; an index outside its range reads memory the call was not given.  Callers that take
 * indices from outside check them first (BNLearnWrapper.with_rows does).  Checked before anything is enqueued: the plain
 * entry point's checks in its order (rows counts among the null pointers, code 10), then after the score argument code 13
 * for set_size < 1, n_sets < 1 or a null set_of with n_sets < batch, then (toggle) the size checks, code 14. */
int dvs_bn_scores_rows(int32_t batch, int32_t n_vars, int32_t n_samples, const uint64_t* data, const uint8_t* card,
                       const uint64_t* parents, int32_t score_type, double score_arg, double* scratch, double* out,
                       int32_t* status, const int32_t* rows, int32_t set_size, int32_t n_sets, const int32_t* set_of,
                       void* stream);
int dvs_bn_toggle_scores_rows(int32_t batch, int32_t n_vars, int32_t n_samples, const uint64_t* data, const uint8_t* card,
                              const uint64_t* parents, int32_t score_type, double score_arg, const int32_t* worklist,
                              double* local, size_t local_bytes, double* toggles, size_t toggles_bytes, int32_t* status,
                              const int32_t* rows, int32_t set_size, int32_t n_sets, const int32_t* set_of, void* stream);

/* Bootstrap draw: rows (device i32 [n_sets][set_size]) with replacement from 0 .. n_samples - 1.  Set r has the global index
 * g = (set_offset + r) mod 2^32 and the key dvs_site_key(seed_lo, seed_hi, 600, g) of csrc/dvs_device.h;
 *   rows[r][i] = (uint64(dvs_draw(key, i)) * n_samples) >> 32
 * (oracle/rng.py restates both functions).  Index k is drawn with probability within 2^-32 of 1 / n_samples, a bias of at
 * most n_samples / 2^32 in all.  A set is a function of (seed, g) only: a request may be cut into calls or shards with
 * set_offset.  Checked in this order: n_sets > 0 (2), set_size >= 1 and n_samples >= 1 (13), n_sets * set_size < 2^31 (2),
 * set_offset >= 0 (12), null pointer (10). */
int dvs_bootstrap_rows(int32_t n_sets, int32_t set_size, int32_t n_samples, uint64_t seed, int64_t set_offset, int32_t* rows,
                       void* stream);

/* Arc counts over a batch of networks (bnlearn's custom.strength with the direction doubled, so that everything stays an
 * integer).  pdag: device u64 [batch][n_vars] in the PDAG form of dvs_cpdag (a DAG's parent masks are one); u and v are
 * adjacent in a network iff bit u of row v or bit v of row u is set.  counts: device i32 [n_vars][n_vars][2], ACCUMULATED into
 * (the caller zeroes it first; chunks and ranks add up).  For every ordered pair u != v and every network in which u and v
 * are adjacent:
 *   counts[u][v][0] += 1
 *   counts[u][v][1] += 2 if the network has u -> v only, 1 if it has u - v, 0 if it has v -> u only
 * so counts[u][v][0] == counts[v][u][0] and counts[u][v][1] + counts[v][u][1] == 2 counts[u][v][0].  Bits on the diagonal or
 * at positions >= n_vars are ignored; the diagonal cells are not written.  Integer adds only: the result does not depend
 * on the order of processing and two runs give equal bytes.  Checked in this order: batch > 0 (2), n_vars in [1, 48] (3),
 * batch * n_vars < 2^31 (2), null pointers (10), counts_bytes < n_vars^2 * 8 (14 with the needed size). */
int dvs_arc_strength(int32_t batch, int32_t n_vars, const uint64_t* pdag, int32_t* counts, size_t counts_bytes, void* stream);

/* Significance threshold and averaged network, one per group.  counts: device i32 [groups][n_vars][n_vars][2] in the layout
 * of dvs_arc_strength; n_networks, min_any: device i32 [groups].  A batch of groups is a threshold sweep over one count matrix
 * (the caller repeats it) or several matrices.  For a pair u < v let A = counts[u][v][0], D = counts[u][v][1] and
 * D' = counts[v][u][1] (counts[v][u][0] is not read).
 *   significance  the pair is significant iff A >= min_any[g].  min_any[g] < 0 asks for the estimated threshold: with
 *                 R = n_networks[g], T = the largest A over the pairs with 2 A <= R, or, when no pair has 2 A <= R, the
 *                 smallest A over all pairs (T = 0 when n_vars = 1: there are no pairs); min_any = T + 1.  This is the L1
 *                 estimator of Scutari and Nagarajan (2013) in closed form: the p minimising the L1 distance between the
 *                 empirical CDF F of the strengths A / R and the step at p is F(1/2), whose type-1 quantile is the largest
 *                 observed strength <= 1/2, or the smallest observed strength when none is.
 *   order         the significant pairs are processed by A descending, then |D - D'| descending, then u n_vars + v ascending.
 *   orientation   u -> v if D > D', v -> u if D < D'; on a tie u -> v is tried first, then v -> u (in an acyclic graph one
 *                 of the two closes no cycle).
 *   insertion     an arc whose head is already an ancestor of its tail would close a cycle and is not added; a pair that
 *                 is not a tie is then dropped.
 * parents: device u64 [groups][n_vars], always acyclic.  info: device i32 [groups][4] = (the min_any used, arcs placed,
 * pairs dropped for a cycle, significant pairs with D == D').  Two differences from bnlearn's averaged.network, on purpose:
 * bnlearn leaves a tie undirected (the result is then a PDAG) where this orients it, and bnlearn finds the threshold with a
 * numerical optimiser (optimize, fuzzy in the last digits) where this takes the closed form; parity with an R run is
 * unpinned and rests on these definitions.  Integers only: two runs give equal bytes.  Checked in this order: groups > 0
 * (2), n_vars in [1, 48] (3), groups * n_vars^2 * 2 < 2^31 (2), null pointers (10), parents_bytes < groups * n_vars * 8 (14
 * with the needed size). */
int dvs_averaged_network(int32_t groups, int32_t n_vars, const int32_t* counts, const int32_t* n_networks,
                         const int32_t* min_any, uint64_t* parents, size_t parents_bytes, int32_t* info, void* stream);

/* The relabelling step of BNLearnWrapper.score (src/problem/bn/bnlearn.py:34-45: graph vertex v stands for data-set variable
 * labels[v]) on the device, from the row codec of dvs_build_records: labels device u8 [B][n_vars], preds device [B][n_vars]
 * (u16, or u64 when preds_are_u64) -> parents device u64 [B][n_vars] in data-set variable indices, ready for dvs_bic_scores.
 * status bit 5 (device int32, zeroed by the caller): the labels of a DAG are not a permutation of 0..n_vars-1 (the reference
 * asserts, bnlearn.py:35); that DAG's masks are zero.  With dvs_encode this keeps the reference's predictor-data pipeline
 * (experiments/01_bn_asia/main.py:268-303: encode -> BIC -> (mu, target) rows) on the device. */
int dvs_bic_parent_masks(int32_t batch, int32_t n_vars, int32_t preds_are_u64, const uint8_t* labels, const void* preds,
                         uint64_t* parents, int32_t* status, void* stream);

/* Predictive mean of the reference's GP predictor (GPRegressionModel, src/predictors/gp.py:13-32:
 * ConstantMean + InducingPointKernel(ScaleKernel(RBFKernel())), evaluated as `model(test_x).mean`,
 * experiments/01_bn_asia/main.py:367-368):  out[b] = constant + outputscale * sum_m alpha[m] exp(-|x_b - z_m|^2 / (2 l^2)).
 * x: device f32 [batch][dim] (encoder means); inducing: device f32 [n_inducing][dim]; alpha: device f64 [n_inducing]
 * (solved once at fit time from the training set, see bic/predictor mirror); out: device f64 [batch].  fp64
 * accumulation.  Parity with gpytorch is unpinned (not installed; no reference predictions exist). */
int dvs_gp_predict(int32_t batch, int32_t n_inducing, int32_t dim, const float* x, const float* inducing,
                   const double* alpha, double outputscale, double lengthscale, double constant, double* out,
                   void* stream);

/* Hyper-parameter training of the same predictor (reference loop: src/predictors/gp.py:55-81 = experiments/01_bn_asia/
 * main.py:329-365, Adam lr 0.01 on -ExactMarginalLogLikelihood(likelihood, model) of the SGPR model): the two kernel-specific
 * steps of one iteration.  The M x M / M x n Cholesky factorisations between them are dense library calls of the host side
 * (dags_vae_search_amd/predictor.py), the parameter update is dvs_clip_adam over the flat [inducing points | 4 raw scalars].
 * dvs_gp_kernel: K [na][nb] (device f64) = outputscale * exp(-|xa_a - xb_b|^2 / (2 lengthscale^2)); xa [na][dim], xb [nb][dim]
 * device f32, dim <= 32.
 * dvs_gp_kernel_backward: G = d objective / d K [na][nb] (device f64) -> dxa [na][dim] (device f64, overwritten):
 * sum_b G'_ab K_ab (xb_b - xa_a) / l^2 with G' = G + G^T when `symmetric` (xa and xb are the same point set, K_uu), else
 * G' = G; row_sums [na][2] (device f64, overwritten): per-row partial sums of d/d lengthscale (sum_b G K d^2 / l^3) and
 * d/d outputscale (sum_b G K / o); the caller adds the rows.  Fixed summation order (bitwise reproducible). */
int dvs_gp_kernel(int32_t na, int32_t nb, int32_t dim, const float* xa, const float* xb, double outputscale,
                  double lengthscale, double* K, void* stream);
int dvs_gp_kernel_backward(int32_t na, int32_t nb, int32_t dim, int32_t symmetric, const float* xa, const float* xb,
                           double outputscale, double lengthscale, const double* G, double* dxa, double* row_sums,
                           void* stream);

/* Acquisition of the same predictor for latent-space Bayesian optimisation (dags_vae_search_amd/search.py; the reference
 * stops before its search, experiments/01_bn_asia/main.py ends at train_predictor).  One launch, `batch` queries x:
 *   mean[b] = constant + k_b . alpha,  var[b] = max(c0 + k_b^T P k_b, 0),  k_b[m] = outputscale exp(-|x_b - z_m|^2 / (2 l^2)),
 *   ei[b]   = imp Phi(imp / sigma) + sigma phi(imp / sigma),  imp = mean[b] - best - xi,  sigma = sqrt(var[b])
 * (expected improvement of a maximisation: bnlearn's BIC, higher is better); sigma <= 1e-12 outputscale: ei = max(imp, 0).
 * grad (nullable): dEI/dx [batch][dim] (device f32) = sum_m (Phi alpha_m + phi / sigma (P k)_m) k_m (z_m - x_b) / l^2
 * (d mean / dx where sigma is below the floor and imp > 0, else 0).  weights: device f64 [n_inducing][ld], ld >= n_inducing
 * + 1: columns 0 .. n_inducing-1 hold the symmetric P, column n_inducing holds alpha (predictor.py: fit_posterior).
 * x: device f32 [batch][dim]; inducing: device f32 [n_inducing][dim]; mean / var / ei: device f64 [batch].  dim <= 32,
 * n_inducing <= DVS_GP_ACQ_MAX_INDUCING (the k block of 16 queries lives in one CU's LDS).  fp64 throughout, the
 * batch x n_inducing kernel matrix is never written to memory; fixed summation order (bitwise reproducible).  (Added in ABI 202 as a
 * pure addition: the version number stays.) */
#define DVS_GP_ACQ_MAX_INDUCING 1023
int dvs_gp_acquire(int32_t batch, int32_t n_inducing, int32_t dim, int32_t ld, const float* x, const float* inducing,
                   const double* weights, double c0, double outputscale, double lengthscale, double constant, double best,
                   double xi, double* mean, double* var, double* ei, float* grad, void* stream);

/* Optional per-kernel timing for the benchmark's roofline leg: while enabled, every kernel launch is bracketed by
 * HIP events recorded on its own stream; dvs_profile_collect waits for them and returns, per kernel name, the
 * number of launches and their summed duration in milliseconds (rows of `name_stride` chars).  Process-global
 * debug state; leave disabled in production. */
void dvs_profile_enable(int on);
int dvs_profile_collect(char* names, int name_stride, int* counts, float* total_ms, int cap);

/* Test hook for the error path: launches an empty kernel with `dynamic_lds_bytes` of dynamic LDS through the same launch
 * macro as every product kernel.  A request above the 160 KB of a gfx950 CU must come back as code 20. */
int dvs_debug_launch(size_t dynamic_lds_bytes, void* stream);

/* Debug/test access: copy saved activation `slot` (natural [B, 16*ceil(n_tokens/16), 64] layout) out of the workspace. */
int dvs_debug_activation(const dvs_shape* s, const void* workspace, int slot, float* out, void* stream);

/* Debug/test access: copy the per-DAG loss terms of the last step out of the workspace: out (device f32 [B][2]) =
 * {reconstruction loss, KL term} of every DAG, the addends of losses[1] and losses[2]. */
int dvs_debug_dag_losses(const dvs_shape* s, const void* workspace, float* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif
