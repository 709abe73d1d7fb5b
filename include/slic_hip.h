/*
 * slic_hip.h — C ABI of libslic_hip.so, the MI355X (gfx950) implementation of SLIC's
 * contrastive-training hot path (R3D-18 encoder fwd/bwd, InfoNCE losses, full-dataset k-means,
 * cosine top-k retrieval).
 *
 * The reference (rvl-lab-utoronto/video_similarity_search) is 100 % Python and has no FFI
 * layer; the library calls it makes on this path — torch.nn.Conv3d /
 * BatchNorm3d (cuDNN), F.cosine_similarity + F.cross_entropy, torch.index_select + bmm,
 * sklearn.cluster.KMeans, sklearn cosine_distances + argsort — are what these entry points
 * replace.  Each declaration cites the reference call site it stands in for
 * (paths relative to the reference repo root).
 *
 * Conventions (all entry points):
 *   - extern "C", return int: 0 = SLIC_OK, negative = error (slic_last_error() gives text,
 *     thread-local).  Nothing throws, nothing allocates or frees caller memory.
 *   - pointers are DEVICE pointers unless the name ends in _host; sizes are elements unless
 *     the name ends in _bytes; `stream` is a hipStream_t passed as void* (NULL = default
 *     stream); all work is asynchronous on that stream.
 *   - workspace: where a function needs scratch memory the caller provides it; the matching
 *     *_workspace_bytes() function gives the size.  Workspaces may be reused across calls on
 *     the same stream.
 *   - fp32 everywhere unless stated; labels/indices int32; row-major.
 */
#ifndef SLIC_HIP_H
#define SLIC_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SLIC_OK 0
#define SLIC_EINVAL -1   /* bad argument / unsupported shape */
#define SLIC_EHIP -2     /* HIP runtime error (launch, memset, ...) */
#define SLIC_ENODEV -3   /* no gfx950 device visible */
#define SLIC_ETIMEOUT -4 /* a bounded wait on a collective ran out (slic_comm_create_timeout, slic_comm_wait): the communicator is aborted */

/* library */
int slic_version(void);                 /* (major<<16)|(minor<<8)|patch */
const char* slic_last_error(void);      /* thread-local, never NULL */
int slic_device_check(void);            /* SLIC_OK iff the current device is gfx950 */

/* ------------------------------------------------------------------------------------------
 * k-means (clustering/cluster_masks.py:64-71 -> sklearn.cluster.KMeans, algorithm 'lloyd';
 * sklearn/cluster/_k_means_lloyd.pyx:168-218, _k_means_common.pyx:167-311, _kmeans.py:174-277,
 * 624-752).  Floating-point contract: oracle/kmeans_oracle.c header.
 * ---------------------------------------------------------------------------------------- */

/* cnorm[j] = k-ascending fmaf chain of c_j.c_j   (row_norms(centers, squared=True),
 * _k_means_lloyd.pyx:98).  C: [K, D] with row stride ldc. */
int slic_kmeans_cnorm(const float* C, int K, int D, int ldc, float* cnorm, void* stream);

/* E-step: labels[i] = argmin_j cnorm[j] - 2*x_i.c_j, strict '<', first index wins
 * (_update_chunk_dense, _k_means_lloyd.pyx:189-213).  X: [N, D] row stride ldx (D % 8 == 0,
 * ldx % 4 == 0, 16-byte aligned).  If labels_old != NULL, *n_changed (int32, device) is
 * incremented by the number of rows whose label differs from labels_old (caller zeroes it).
 * best_score (optional, [N]) receives the winning score.
 * A row none of whose scores compares below +inf (a NaN among its values makes every score NaN; an infinity can make every
 * score +inf) gets label 0, as sklearn's argmin does; the winning score of such a row is not specified.  Every other row is
 * unaffected. */
size_t slic_kmeans_assign_workspace_bytes(int64_t N, int K);
int slic_kmeans_assign(const float* X, int64_t N, int D, int ldx, const float* C, int K, int ldc,
                       const float* cnorm, int32_t* labels, const int32_t* labels_old,
                       int32_t* n_changed, float* best_score, void* workspace, void* stream);

/* The same E-step on operands whose rows are already in the MFMA's LDS order — inside every group of eight k's,
 * [k0 k2 k4 k6 | k1 k3 k5 k7] (slic_kmeans_permute_k8; the centres can come permuted out of slic_kmeans_finalize) — so
 * both tiles go HBM -> LDS by DMA.  Same arithmetic, bit-identical labels; same workspace size. */
int slic_kmeans_permute_k8(const float* X, int64_t N, int D, int ldx, float* Xp, int ldxp, void* stream);
int slic_kmeans_assign_perm(const float* Xp, int64_t N, int D, int ldxp, const float* Cp, int K, int ldcp,
                            const float* cnorm, int32_t* labels, const int32_t* labels_old,
                            int32_t* n_changed, float* best_score, void* workspace, void* stream);
/* Which kernels slic_kmeans_assign_perm (and the E-step inside slic_kmeans_lloyd_step / _lloyd_local) runs for a shape on the
 * current device: the launch and this query call one decision function.  No device work, but the compute-unit count of the
 * current device is part of the decision: without a device this returns an error with a message.
 * out[6] = {route: 0 = 128 x 64 DMA tile, 1 = centroids in registers; k-tiles of 32 per point tile of the register kernel
 * (4 / 8 / 16, else 0); point slices (gridDim.x of the register kernel, else 0); centroid blocks (gridDim.y); partial lists the
 * combine pass reads; the compute-unit count used}. */
int slic_kmeans_assign_perm_plan(int64_t N, int K, int D, int ldxp, int* out /* [6] */);

/* M-step sums: sums[j,:] = sum of rows with label j, fp32, ASCENDING ROW ORDER (deterministic;
 * == sklearn's centers_new[label] += X[i] loop on one thread, _k_means_lloyd.pyx:215-218);
 * counts[j] = member count as float (weight_in_clusters). */
size_t slic_kmeans_accumulate_workspace_bytes(int64_t N, int K);
int slic_kmeans_accumulate(const float* X, int64_t N, int D, int ldx, const int32_t* labels,
                           int K, float* sums, float* counts, void* workspace, void* stream);

/* sums/counts <- sum over shards s = 0..n_shards-1 (in that order) of partial_sums + s*shard_stride
 * ([K*D] each) and partial_counts + s*shard_stride ([K] each): the fixed-order combine after an
 * all-gather of per-GPU partials (== sklearn's per-thread buffers reduced in
 * thread order, _k_means_lloyd.pyx:142-152). */
int slic_kmeans_combine_shards(const float* partial_sums, const float* partial_counts,
                               int64_t shard_stride, int n_shards, int K, int D, float* sums,
                               float* counts, void* stream);

/* dist[i] = k-ascending fmaf chain of (x_ik - C[labels[i],k])^2 (used by empty-cluster
 * relocation, _k_means_common.pyx:183, and inertia, _k_means_common.pyx:103-128). */
int slic_kmeans_dist_to_assigned(const float* X, int64_t N, int D, int ldx, const float* C,
                                 int ldc, const int32_t* labels, float* dist, void* stream);

/* inertia = sum_i dist[i] in double (256-row blocks summed in order, then blocks in order). */
size_t slic_sum_f32_to_f64_workspace_bytes(int64_t N);
int slic_sum_f32_to_f64(const float* v, int64_t N, double* out, void* workspace, void* stream);

/* _relocate_empty_clusters_dense (_k_means_common.pyx:167-211), in two steps so that a sharded
 * run can merge candidates across GPUs in between:
 *  select_far: the n_sel farthest rows by (dist descending, ties -> lower row); dist is clobbered.
 *              (sklearn: np.argpartition(distances, -n_empty)[:-n_empty-1:-1]; identical for
 *              n_empty == 1, introselect-order-dependent above that.)  A taken row's dist becomes -2, every other entry
 *              stays.  Only a distance that compares greater than -1 can be taken, so a NaN never is; when such rows
 *              run out (n_sel > N, NaNs) the remaining entries are far_idx = N and far_dist = -1.  N < 2^31.
 *  apply_relocation: for e = 0..n-1 in order: sums[old_ids[e]] -= xfar[e]; sums[new_ids[e]] = xfar[e];
 *              counts[new] = 1; counts[old] -= 1.   xfar: [n, D] rows (stride ldf). */
int slic_kmeans_select_far(float* dist, int64_t N, int n_sel, int32_t* far_idx, float* far_dist,
                           void* stream);
int slic_kmeans_apply_relocation(const float* xfar, int ldf, const int32_t* old_ids,
                                 const int32_t* new_ids, int n, int D, float* sums, float* counts,
                                 void* stream);

/* _average_centers + _center_shift (_k_means_common.pyx:274-311): C_new = sums * (1/counts)
 * (empty clusters copy the biggest one, in sklearn's in-place order), shift[j] =
 * ||C_new_j - C_old_j||; cnorm_new (optional, [K]) = slic_kmeans_cnorm(C_new), so the next E-step needs no extra
 * launch.  status (device double[4]) = { sum_j shift[j]^2, number of clusters with
 * counts == 0, *n_changed (or -1 if NULL), 0 } — the one word the host loop reads per iteration
 * (_kmeans.py:717-731).  C_new must not alias sums or C_old.
 * The biggest cluster is the FIRST maximum of counts (np.argmax); an empty cluster j copies its row — the mean when it
 * precedes j, the raw sum otherwise.  With every count zero that is cluster 0 unscaled: every row of C_new is sums[0].
 * shift[j] = sqrtf(groups of four squared differences, each added left to right, groups ascending, then the D % 4 tail),
 * every product and sum rounded on its own (no fused multiply-add); status[0] adds shift[j]^2 in double over a fixed
 * partition (thread t of 256: j = t, t + 256, ...) and a fixed binary tree. */
int slic_kmeans_finalize(const float* C_old, const float* sums, const float* counts, int K, int D,
                         float* C_new, float* shift /* [K] */, float* cnorm_new /* [K] or NULL */,
                         float* C_new_perm /* [K][D] in slic_kmeans_permute_k8 order, or NULL */,
                         int spherical /* 1: C_new rows are L2-normalised means (spherical k-means,
                                          clustering/cluster_masks.py:73-77 -> spherecluster) */,
                         const int32_t* n_changed, double* status, void* stream);

/* One whole single-GPU Lloyd iteration enqueued by one call: *n_changed = 0; slic_kmeans_assign_perm(Xp, Cp_old,
 * cnorm_old -> labels, n_changed vs labels_old); slic_kmeans_accumulate(X, labels -> sums, counts);
 * slic_kmeans_finalize(-> C_new, Cp_new, cnorm_new, shift, status).  X / Xp share ldx; the centre matrices are dense
 * [K][D].  (A sharded fit calls the three pieces itself, with the all-gather between the last two.) */
size_t slic_kmeans_lloyd_step_workspace_bytes(int64_t N, int K);
int slic_kmeans_lloyd_step(const float* X, const float* Xp, int64_t N, int D, int ldx, const float* C_old,
                           const float* Cp_old, const float* cnorm_old, int K, int32_t* labels,
                           const int32_t* labels_old, int32_t* n_changed, float* sums, float* counts,
                           float* C_new, float* Cp_new, float* cnorm_new, float* shift, int spherical,
                           double* status, void* workspace, void* stream);

/* The SHARDED Lloyd iteration (rows of X split over the ranks, centres replicated) as two calls around its ONE collective —
 * the GPU form of what the reference does on rank 0 while the other ranks wait in a barrier (online_train.py:625-662), with the
 * exchange SURVEY.md §8e row 2 specifies: one message [K*D sums | K counts | n_changed] per iteration.
 *   slic_kmeans_lloyd_local : *n_changed = 0; slic_kmeans_assign_perm on this rank's rows; slic_kmeans_accumulate into `payload`
 *       = [K*D sums | K counts | n_changed & 0xFFFFF | n_changed >> 20]  (K*D + K + 2 numbers; fp32, or — payload_f64 — the same
 *       fp32 results widened to double: the operand of an fp64 all-reduce, whose sum of <= 2^29-apart fp32 values is exact and
 *       therefore independent of RCCL's reduction order).
 *   (caller) all-gather of the fp32 payloads [n_parts][stride], or all-reduce(sum) of the fp64 payload (n_parts = 1).
 *   slic_kmeans_lloyd_global: sums / counts = the payloads added in part order (fp32), or the reduced fp64 payload rounded to
 *       fp32; then slic_kmeans_finalize on them (status[2] = the summed n_changed).  sums / counts are also written out
 *       (empty-cluster relocation reads them). */
size_t slic_kmeans_lloyd_local_workspace_bytes(int64_t N, int K);
int slic_kmeans_lloyd_local(const float* X, const float* Xp, int64_t N, int D, int ldx, const float* Cp_old,
                            const float* cnorm_old, int K, int32_t* labels, const int32_t* labels_old, void* payload,
                            int payload_f64, void* workspace, void* stream);
int slic_kmeans_lloyd_global(const void* parts, int parts_f64, int64_t stride, int n_parts, const float* C_old, int K, int D,
                             float* sums, float* counts, float* C_new, float* Cp_new, float* cnorm_new, float* shift,
                             int spherical, double* status, void* stream);

/* The certified bf16 E-step: the score GEMM runs on the bf16 MFMA over round-to-nearest-even images of the rows and
 * only NOMINATES centroids — those whose coarse score minus its proven error bound is not above the smallest coarse score plus bound;
 * a row with several nominees takes the argmin of their exact scores (the fmaf chain of slic_kmeans_assign, natural column order,
 * first index wins).  Labels, n_changed and everything downstream are bit-identical to the fp32 entry points; the bf16 scores never
 * reach an output (there is no best_score: callers that want one use slic_kmeans_assign).
 * Domain: D % 8 == 0, D <= 512, N < 2^31; outside it these calls return SLIC_EINVAL with a message — they never switch precision.
 *   slic_kmeans_bf16_plan : host only.  out[6] = {inside the domain (0 / 1), columns of an image row (D rounded up to 16), pair slots
 *       per (row, 128-centroid block), 128-centroid blocks, bytes of the image of N rows, bytes of the image of K rows}.
 *   slic_kmeans_bf16_eps  : the relative bound of |bf16-MFMA dot - fp32 dot| / (||x|| ||c||), the constant of slic_cosine_topk_bf16_eps.
 *   slic_kmeans_bf16_image: image[N][Dp] (bf16, dense rows, zero padding) of X[N][D] (rows ldx floats apart) and, when norms is not
 *       NULL, norms[i] = ||x_i||.  The image and norms of the centred data are made once per fit.
 *   slic_kmeans_assign_bf16: labels of X against C (natural column order, NOT the k8-permuted copies) from the images Xb / Cb, the row
 *       norms and cnorm (slic_kmeans_cnorm of C).  labels_old / n_changed as slic_kmeans_assign (*n_changed is added to).
 *       stats (or NULL): int32[3] on the device, ADDED to: {rows whose label came from exact rescoring, rows among them whose slots
 *       overflowed and that ran the exact chain over all K centroids, nominees of all rows (K for an overflowed row)}.
 *   slic_kmeans_lloyd_step_bf16 / slic_kmeans_lloyd_local_bf16: slic_kmeans_lloyd_step / slic_kmeans_lloyd_local with this E-step inside.
 *       Cb is SCRATCH of K x Dp bf16 values: the call writes C_old's image there.  The M-step, the payload layout and
 *       slic_kmeans_lloyd_global are unchanged. */
int slic_kmeans_bf16_plan(int64_t N, int K, int D, int64_t* out /* [6] */);
float slic_kmeans_bf16_eps(void);
int slic_kmeans_bf16_image(const float* X, int64_t N, int D, int ldx, void* image, float* norms, void* stream);
size_t slic_kmeans_assign_bf16_workspace_bytes(int64_t N, int K);
int slic_kmeans_assign_bf16(const float* X, const void* Xb, const float* xnorm, int64_t N, int D, int ldx, const float* C,
                            const void* Cb, const float* cnorm, int K, int ldc, int32_t* labels, const int32_t* labels_old,
                            int32_t* n_changed, int32_t* stats, void* workspace, void* stream);
size_t slic_kmeans_lloyd_step_bf16_workspace_bytes(int64_t N, int K);
int slic_kmeans_lloyd_step_bf16(const float* X, const float* Xp, const void* Xb, const float* xnorm, int64_t N, int D, int ldx,
                                const float* C_old, void* Cb, const float* cnorm_old, int K, int32_t* labels,
                                const int32_t* labels_old, int32_t* n_changed, float* sums, float* counts, float* C_new,
                                float* Cp_new, float* cnorm_new, float* shift, int spherical, double* status, int32_t* stats,
                                void* workspace, void* stream);
size_t slic_kmeans_lloyd_local_bf16_workspace_bytes(int64_t N, int K);
int slic_kmeans_lloyd_local_bf16(const float* X, const float* Xp, const void* Xb, const float* xnorm, int64_t N, int D, int ldx,
                                 const float* C_old, void* Cb, const float* cnorm_old, int K, int32_t* labels,
                                 const int32_t* labels_old, void* payload, int payload_f64, int32_t* stats, void* workspace,
                                 void* stream);

/* The collective of the sharded iteration behind the C ABI: an opaque RCCL communicator, created and destroyed explicitly (the
 * library's only global state besides the last-error string), and an in-place sum all-reduce on the caller's stream — a thin wrapper
 * over ncclAllReduce (RCCL over xGMI; bound at first use with dlopen, no link-time dependency).  One process per GPU: rank 0 calls
 * slic_comm_unique_id and hands the SLIC_COMM_ID_BYTES bytes to the other ranks (any channel: torch.distributed, a file, MPI), then
 * every rank calls slic_comm_create on its device.  Stands in for the NCCL group the reference sets up in
 * misc/distributed_helper.py:8-26 where the path needs its one exchange (online_train.py:625-662 -> SURVEY.md §8e row 2). */
#define SLIC_COMM_ID_BYTES 128
typedef struct slic_comm slic_comm;
int slic_comm_unique_id(void* id_out /* SLIC_COMM_ID_BYTES */);
int slic_comm_create(const void* id, int world, int rank, slic_comm** out);
/* The same with a deadline (milliseconds; 0 = none): the communicator is created non-blocking and polled; if the peers have not all
 * joined in time — a rank died before the rendezvous, a wrong world size — it is aborted and SLIC_ETIMEOUT comes back instead of a
 * hang.  The deadline also bounds the enqueue of every later slic_allreduce_* of this communicator. */
int slic_comm_create_timeout(const void* id, int world, int rank, int timeout_ms, slic_comm** out);
int slic_allreduce_f32(slic_comm* comm, float* buf, int64_t n, void* stream);
int slic_allreduce_f64(slic_comm* comm, double* buf, int64_t n, void* stream);
/* Bounded wait for the collectives already enqueued: returns when everything enqueued on `stream` so far has run (SLIC_OK), when RCCL
 * reports an asynchronous error (SLIC_EHIP), or when timeout_ms (0 = none) has passed (SLIC_ETIMEOUT: a peer never joined) — in the two
 * failure cases the communicator has been ABORTED (its stuck kernel is released, every later call on it fails) so that the rank can
 * exit non-zero instead of hanging its peers' job.  What torch.distributed's process-group timeout is to the reference's collectives
 * (misc/distributed_helper.py:30-64). */
int slic_comm_wait(slic_comm* comm, void* stream, int timeout_ms);
/* The same bounded wait on ONE event (a hipEvent_t the caller recorded behind the work it wants finished — the sharded Lloyd loop records
 * one behind every iteration's collective + status read-back and waits for iteration `it` while iteration `it + 1` is already enqueued:
 * slic_comm_wait would drain that one too). */
int slic_comm_wait_event(slic_comm* comm, void* event, int timeout_ms);
/* give up on a communicator at once (ncclCommAbort) and free the handle: never blocks (what a process-exit hook calls) */
int slic_comm_abort(slic_comm* comm);
/* orderly teardown: ncclCommFinalize, polled to completion under the communicator's deadline (10 s when it has none), then
 * ncclCommDestroy; a lost peer or an asynchronous error ends in ncclCommAbort (SLIC_ETIMEOUT / SLIC_EHIP).  The handle is freed either way. */
int slic_comm_destroy(slic_comm* comm);

/* The same exchange as a ONE-SHOT all-to-all over peer-mapped device memory (csrc/oneshot.hip): where the ring all-reduce above is 2 (W - 1)
 * dependent steps over xGMI's point-to-point links, every rank here WRITES its payload into an inbox of each peer at once (one link per
 * peer), raises a flag per 32 KB chunk, waits for its peers' flags and adds the W payloads it then holds in rank order — one kernel per
 * exchange, no RCCL.  Sums are fp64 (exact for the k-means payload: every rank ends with bit-identical numbers).  Replaces the rank-0
 * k-means + barrier of online_train.py:625-662 together with slic_kmeans_lloyd_local / _global; process model of
 * misc/distributed_helper.py:30-37 (one process per GPU; two processes may also share ONE GPU, which is how a one-GPU box tests it).
 *   slic_oneshot_create : allocates the rank's inbox for payloads of up to max_n doubles (uncached device memory) on the current device
 *                         and writes its IPC handle (SLIC_IPC_HANDLE_BYTES) to handle_out; timeout_ms bounds every wait of an exchange
 *                         (0 = none);
 *   (caller)            : gathers the W handles in rank order over any channel (torch.distributed, a file, MPI);
 *   slic_oneshot_connect: maps the peers' inboxes (hipIpcOpenMemHandle; needs HSA_ENABLE_IPC_MODE_LEGACY=0 on this driver);
 *   slic_allreduce_oneshot_f64: in-place sum of n doubles (buf 16-byte aligned) across the ranks, asynchronous on `stream`; every
 *                         rank must issue the same sequence of exchanges with the same n;
 *   slic_oneshot_check  : once the stream (or an event behind the exchange) has completed — SLIC_OK, or SLIC_ETIMEOUT when a wait ran out:
 *                         a peer never pushed (lost rank).  The kernel itself never hangs: it gives up after timeout_ms, records the
 *                         exchange number in a host-mapped word and finishes; the payloads since are garbage and the caller must raise.
 *   slic_oneshot_info   : out[4] = {world, rank, memory kind (0 uncached, 1 fine-grained, 2 plain device memory), exchanges issued}. */
#define SLIC_IPC_HANDLE_BYTES 64
typedef struct slic_oneshot slic_oneshot;
int slic_oneshot_create(int world, int rank, int64_t max_n, int timeout_ms, slic_oneshot** out, void* handle_out /* SLIC_IPC_HANDLE_BYTES */);
int slic_oneshot_connect(slic_oneshot* c, const void* all_handles /* world x SLIC_IPC_HANDLE_BYTES, rank order */);
int slic_allreduce_oneshot_f64(slic_oneshot* c, double* buf, int64_t n, void* stream);
int slic_oneshot_check(slic_oneshot* c);
int slic_oneshot_info(const slic_oneshot* c, int* out /* [4] */);
int slic_oneshot_destroy(slic_oneshot* c);

/* column sums / sums of squares in double (rows ascending in 1024-row segments, segments in
 * order) — X.mean(axis=0) and np.var(X, axis=0) of KMeans.fit / _tolerance
 * (_kmeans.py:1479-1481, 279-288). */
size_t slic_col_stats_workspace_bytes(int64_t N, int D);
int slic_col_stats(const float* X, int64_t N, int D, int ldx, double* col_sum, double* col_sumsq,
                   void* workspace, void* stream);

/* out[i,:] = X[i,:] - v  (X -= X_mean, _kmeans.py:1481) */
int slic_sub_rowvec(const float* X, int64_t N, int D, int ldx, const float* v, float* out,
                    int ldo, void* stream);

/* out[i,:] = X[i,:] / ||X[i,:]||_2   (preprocess_features_kmeans, cluster_masks.py:30-34;
 * no epsilon, like the reference): out = x / float32(sqrt(sum of x^2 in double)), a true division.  An all-zero row
 * gives 0 / 0: a row of NaN, as torch's x / x.norm() does.  Any D and strides >= D. */
int slic_l2norm_rows(const float* X, int64_t N, int D, int ldx, float* out, int ldo, void* stream);

/* k-means++ helper (_kmeans.py:236-264): for T candidate rows cand[t] of X,
 * newdist[t,i] = min(closest[i], ||x_i - x_cand[t]||^2) and pot[t] = sum_i newdist[t,i] (double).
 * If closest == NULL (the first centre, T == 1; any T is taken): newdist[t,i] = ||x_i - x_cand[t]||^2.
 * The squared distance is the k-ascending fmaf chain of (x_i - x_cand[t])^2 (slic_kmeans_dist_to_assigned's chain); the
 * order of pot's double sum is not fixed.  1 <= T <= 16, D % 4 == 0, ldx >= D, T * D * 4 <= 64 KiB, 0 < N < 2^31. */
size_t slic_kmeanspp_step_workspace_bytes(int64_t N, int T);
int slic_kmeanspp_step(const float* X, int64_t N, int D, int ldx, const int32_t* cand, int T,
                       const float* closest, float* newdist, double* pot, void* workspace,
                       void* stream);
/* k-means++ seeding (_kmeans_plusplus, _kmeans.py:174-277) as ONE enqueued sequence: centre 0 = row `first`; for
 * c = 1..K-1: T candidates = searchsorted(cumsum(closest), uniforms[(c-1)*T + t] * current_pot) (clipped), squared distances
 * of every row to them, min with closest, potentials in double, first-minimum candidate kept.  `uniforms` (device,
 * [(K-1)*T] doubles in [0, 1)) are the host RNG's draws — the draws do not depend on the data, so the host never waits.
 * K == 1 has no draws: uniforms is not read and may be NULL (in slic_kmeanspp_run_batch too).
 * idx_out (device, [K]) receives the chosen row indices. */
size_t slic_kmeanspp_run_workspace_bytes(int64_t N, int T);
int slic_kmeanspp_run(const float* X, int64_t N, int D, int ldx, int first, int K, int T, const double* uniforms,
                      int32_t* idx_out,
                      const float* Xp /* optional: slic_kmeans_permute_k8(X), same ldx */,
                      const float* xnorm /* optional: [N] squared row norms; with Xp the distances run on the matrix
                                            pipe as |x|^2 + |c|^2 - 2 x.c (sklearn's euclidean_distances form) */,
                      void* workspace, void* stream);
/* The R initialisations of KMeans(n_init = R) (the n_init loop of KMeans.fit, _kmeans.py:1500-1530, as
 * clustering/cluster_masks.py:70-71 calls it) seeded in lock-step: firsts[r] (HOST array) = run r's first row, uniforms (device,
 * [R][K-1][T] doubles: the host RNG's draws in the order the sequential loop makes them), idx_out (device, [R][K]).  One pass
 * over X per centre for all runs together; every run's arithmetic is that of slic_kmeanspp_run (bit-identical picks).  Xp = the
 * k-permuted copy (slic_kmeans_permute_k8), xnorm = its squared row norms; R * T <= 160. */
size_t slic_kmeanspp_run_batch_workspace_bytes(int64_t N, int T, int R);
int slic_kmeanspp_run_batch(const float* Xp, const float* xnorm, int64_t N, int D, int ldx, int R, const int32_t* firsts, int K, int T,
                            const double* uniforms, int32_t* idx_out, void* workspace, void* stream);

/* inclusive prefix sum of v (float) in double, and searchsorted(cumsum, vals[t], 'left')
 * clipped to N-1  (stable_cumsum + np.searchsorted, _kmeans.py:243-248).  'left': the FIRST index whose prefix sum
 * reaches vals[t] (>=), so a value equal to a prefix sum that a run of zeros repeats gives the run's first row, and
 * vals[t] <= 0 gives 0; a value above the total gives N - 1 (the clip).  N < 2^31, T > 0. */
size_t slic_cumsum_search_workspace_bytes(int64_t N);
int slic_cumsum_search(const float* v, int64_t N, const double* vals, int T, int32_t* idx_out,
                       void* workspace, void* stream);

/* ------------------------------------------------------------------------------------------
 * 3-D convolution / linear layers as a table-driven gather-GEMM on fp32 MFMA
 * (models/resnet.py:11-25,126-131 nn.Conv3d forward + autograd dgrad/wgrad -> cuDNN in the
 * reference; models/resnet.py:182-184 nn.Linear).  Activations are NDHWC fp32
 * ([B, T, H, W, C], C % 4 == 0), weights packed K-contiguous.  See csrc/conv.hip.
 * ---------------------------------------------------------------------------------------- */
typedef struct SlicConvArgs {
  const float* src;        /* gathered operand: [B, Ts, Hs, Ws, Cs] */
  const float* wgt;        /* packed weights [N][ldw], k = table column (conv_gemm only) */
  float* dst;              /* output (conv_gemm only) */
  const int32_t* tab;      /* [nchunks][4] per 16-byte K-chunk: {src element delta,
                              tap mask (1<<(oa+3)) | (1<<(7+ob+3)) | (1<<(14+oc+3)) for tap offsets |o| <= 3, or -1 = all-zero chunk,
                              weight column of the chunk,
                              packed tap offsets (oa+128) | (ob+128)<<8 | (oc+128)<<16} */
  const int32_t* tap_tab;  /* optional [ntaps][4] per-TAP records {src element delta, tap mask, weight column base, 0} for the
                              LDS-DMA variants (needs Cs % 32 == 0, K = ntaps * Cs exactly); NULL otherwise */
  const float* bias;       /* [N] or NULL */
  const float* scale;      /* [N] or NULL: v = v*scale + shift (eval-mode BatchNorm) */
  const float* shift;      /* [N] or NULL */
  const float* addend;     /* same addressing as dst, or NULL: v += addend (residual / grad accumulate) */
  float* stat_partial;     /* [ceil(M/tile_m)][2][N] per-workgroup (sum, sum (v - mean_wg)^2) of v = acc+bias, or NULL */
  int64_t M;               /* rows = B * Ga * Gb * Gc */
  uint32_t src_bytes;      /* size of the src tensor in bytes (< 4 GiB: loads are range-checked buffer loads) */
  uint32_t wgt_bytes;      /* size of the packed weight matrix in bytes */
  int N;                   /* output channels */
  int nchunks;             /* K / 4, multiple of 8 */
  int Cs, Ts, Hs, Ws;      /* source dims */
  int Ga, Gb, Gc;          /* output grid per batch item */
  int sa, sb, sc;          /* source coordinate of grid point g = g*s (+ tap offset) */
  int ldw, ldo;            /* weight row stride, dst row stride (elements) */
  int dst_strided;         /* 0: dst row = m; 1: dst row = ((b*Da + ga*da+ea)*Db + gb*db+eb)*Dc + gc*dc+ec */
  int Da, Db, Dc, da, db, dc, ea, eb, ec;
  int relu;                /* clamp at 0 last */
  const float* mask_src;   /* optional, same addressing as dst: v = mask_src > 0 ? v : 0 after the addend (ReLU backward of the
                              layer that consumes this gradient) */
  const float* bwd_z;      /* optional, same addressing as dst: with bwd_mean / bwd_invstd ([N]) and bwd_partial, the epilogue
                              also emits the BatchNorm-backward partial sums of the stored gradient v: */
  const float* bwd_mean;
  const float* bwd_invstd;
  float* bwd_partial;      /* [ceil(M/tile_m)][2][N]: per workgroup (sum v, sum v * (bwd_z - mean) * invstd); NULL = off */
  const uint32_t* row_tab; /* optional [M][2] per-row records {byte offset of the row's source origin, 21-bit in-bounds mask}
                              written by slic_conv_row_table; slic_conv_wgrad's LDS-DMA kernel then does no per-row
                              coordinate arithmetic.  NULL: the kernel decodes rows itself */
  int k_run_len;           /* 0: K = taps x Cs, one pixel per tap (Cs % 4 == 0).  > 0: "W-run" operand for few-channel inputs
                              (the RGB stem): src is [B, Ts, Hs, Ws, Cs] with ANY Cs (3) and Ws already zero-padded along W; K is
                              cut into runs of k_run_len floats (a multiple of 4) = k_run_px consecutive pixels x Cs channels of one
                              (kt, kh) tap row, padded with zero-weight floats: 7 x 3 = 21 -> 24 instead of 7 x 4 = 28 */
  int k_run_px;            /* real pixels (kw taps) per run; run r covers taps r * k_run_px ... (slic_conv_wgrad unpacks with it) */
} SlicConvArgs;

/* rows per workgroup of the tile slic_conv_gemm runs for (args, variant) — sizes stat_partial / bwd_partial.  Variants:
 * 0 = register-staged 64 x 64 tiles (any source channel count: per-chunk table `tab`); 20 / 22 = LDS-DMA ring, 64 x 64 / 128 x 64 tiles
 * (per-tap table `tap_tab`, Cs % 32 == 0); 30 = Winograd F(4, 3) along W; 31 = Winograd F(4, 3) x F(2, 3) over (W, H) (see
 * slic_pack_weight_wino / slic_pack_weight_wino2). */
int slic_conv_tile_m(const SlicConvArgs* args, int variant);
/* dst = epilogue(gather(src) x wgt^T): forward conv, data gradient, linear. */
int slic_conv_gemm(const SlicConvArgs* args, int variant, void* stream);
/* n (<= 8) independent GEMMs with the same N in ONE launch (blockIdx.z picks the GEMM): the parity classes of a stride-2
 * data gradient, whose K loops are too short (1-8 taps) to fill the chip one launch at a time.  Variants 20 and 22. */
int slic_conv_gemm_multi(const SlicConvArgs* args, int n, int variant, void* stream);
/* Tail-split launch of the same GEMM (variants 20 and 22): row blocks [0, nfull_rb) run whole; the remaining ones — what
 * would be a last, partly filled round of the chip's residency slots — are cut `splits` ways along K into the same grid and
 * finished (pieces added in split order, then the ordinary epilogue) by a second pass over those rows only.  nfull_rb = 0 is plain
 * split-K (raw accumulators to workspace[splits][M][N]); splits <= 1 forwards to slic_conv_gemm.  Deterministic.  Stands in for cuDNN's algorithm choice on
 * the few-tile layers of models/resnet.py:126-131 (layer3 / layer4 at small M).
 * Variant 31 (two-dimensional Winograd): nfull_rb counts 64-TILE blocks; the blocks behind them cut their K loop — the 3 Cs / 8 double
 * stages in (channel group, kt) order — into `splits` even pieces (splits must divide 3 Cs / 16, 2 .. 16: SLIC_EINVAL otherwise, and a
 * workspace size of 0) and a finish pass adds the pieces in order and runs the epilogue; splits <= 1 is the plain launch. */
size_t slic_conv_gemm_tailsplit_workspace_bytes(const SlicConvArgs* args, int variant, int nfull_rb, int splits);
int slic_conv_gemm_tailsplit(const SlicConvArgs* args, int variant, int nfull_rb, int splits, void* workspace, void* stream);

/* dW[N][C][ntaps] (reference layout) = sum_m gather(src)[m, tap*Cs + c] * dy[m, n]; `splits` slices of
 * m reduced in fixed order.  args->wgt/dst unused. */
size_t slic_conv_wgrad_workspace_bytes(const SlicConvArgs* args, int splits);
int slic_conv_wgrad(const SlicConvArgs* args, const float* dy, int ldy, int splits, int C, int ntaps,
                    float* dW, void* workspace, void* stream);
/* row_tab[m] = {(((b*Ts + ga*sa)*Hs + gb*sb)*Ws + gc*sc)*Cs*4, bit (7*dim + o + 3) set iff coordinate + o is inside the
 * source for o in -3..3} for the M rows of args' geometry (args->src etc. unused): 8 bytes per row. */
int slic_conv_row_table(const SlicConvArgs* args, uint32_t* row_tab, void* stream);
/* Wp[n][tap*Cs + c] = W[n][c][tap] for c < C — forward operand.  The padding (channels C..Cs, columns ntaps*Cs..Kp) is NOT
 * written: the caller zeroes the operand once when it allocates it (same for Wd below: rows C..Cs, columns ntaps*N..Kd). */
int slic_pack_weight_fwd(const float* W, int N, int C, int ntaps, int Cs, int Kp, float* Wp, void* stream);
/* W-run operand (SlicConvArgs.k_run_len): Wp[n][run * run_len + px * C + c] = W[n][c][run * run_px + px], zero elsewhere */
int slic_pack_weight_fwd_runs(const float* W, int N, int C, int ntaps, int run_len, int run_px, int Kp, float* Wp, void* stream);
/* Wd[c][tap*N + n] = W[n][c][tap] (Cs rows, Kd columns) — data-gradient operand */
int slic_pack_weight_dgrad(const float* W, int N, int C, int ntaps, int Cs, int Kd, float* Wd, void* stream);
/* Operand of slic_conv_gemm variant 30 — Winograd F(4, 3) along W for the 3 x 3 x 3 / stride 1 / pad 1 layers (what cuDNN's
 * algorithm search may pick behind nn.Conv3d, models/resnet.py:11-17, online_train.py:444): U_p = sum_kw G[p][kw] w[..][kw] for the
 * six points p, laid out in the kernel's LDS stage order
 *   U[(((tap9 * C_/8 + cc) * N_/64 + nb) * 12 + p * 2 + h) * 64 + nl][j],  tap9 = kt * 3 + kh, n = 64 nb + nl, c = 8 cc + 4 h + j.
 * dgrad = 0: forward operand (N_ = N outputs, C_ = C reduction channels); dgrad = 1: data-gradient operand (N_ = C, C_ = N, taps
 * flipped).  9 * C * N * 6 floats.  Needs N_ % 64 == 0 and C_ % 8 == 0.  Variant 30 itself: same SlicConvArgs as the other
 * variants (stride-1 same-size geometry, no bias), wgt / wgt_bytes = this operand; Ws % 4 == 0, or — the last tile of a row ragged —
 * a padded width 4 ceil(Ws / 4) that divides 128; slab rows of slic_conv_tile_m(args, 30) GEMM rows (128, or 128 / Wp * Ws). */
int slic_pack_weight_wino(const float* W, int N, int C, int dgrad, float* U, void* stream);
/* Variant 31 of slic_conv_gemm: Winograd in TWO dimensions, F(4, 3) along W x F(2, 3) along H — 24 multiplies per (kt, c, n) and tile of
 * 2 x 4 outputs where the direct form has 72 and variant 30 has 36, all exact-fp32 MFMA.  Same SlicConvArgs as variant 30 (stride-1
 * same-size 3 x 3 x 3 geometry, no bias, Cs = 64 x a power of two, N % 64 == 0); wgt / wgt_bytes = the operand written here:
 * U2[kt][C/4][N/64][Hpoint 4][Wpoint 6][column half 2][channel pair 2][n 32][2 ch] = Gh w Gw^T, 3 * 24 * C * N floats (dgrad = 1: flipped / transposed for the data
 * gradient).  Stands in for the same cuDNN calls as variant 30 (models/resnet.py:11-17, 41-57).  Blocks of 64 tiles must all hold the
 * same number of real outputs — slic_conv_tile_m(args, 31) returns it (the slab rows' size) or 0 when the geometry does not allow
 * it: H even and W % 4 == 0, or H even and ceil(W / 4) | 64, or ceil(H / 2) * ceil(W / 4) | 64. */
int slic_pack_weight_wino2(const float* W, int N, int C, int dgrad, float* U, void* stream);
/* Weight gradient by the transposed TWO-dimensional algorithm, dW = Gh^T [sum over tiles of (Bh^T x Bw) . (Ah dY Aw^T)] Gw: 24
 * multiplies per (kt, c, n) and tile of 2 x 4 outputs (slic_conv_wgrad_wino: 36, the direct form: 72); replaces slic_conv_wgrad_wino
 * where variant 31 runs the forward (any H, W: ragged tiles are masked).  args as slic_conv_wgrad_wino; tile_tab: (M / (Hs Ws)) *
 * ceil(Hs / 2) * ceil(Ws / 4) records of 8 bytes written once per geometry by slic_conv_wino2_tile_table; `splits` slices of the
 * tiles, reduced in a fixed order (deterministic: groups of consecutive slices, then the groups); workspace: splits x 3 x 12 x Cs x N floats (the
 * W-points are taken back through Gw before they leave the kernel).  One workgroup per (kt, 64 x 64 block,
 * slice) holding ALL FOUR H-points: 3 x Cs / 64 x N / 64 x splits workgroups of 512 threads, one per CU.  Limits (SLIC_EINVAL beyond them;
 * models/conv_plan.py keeps such shapes on slic_conv_wgrad_wino / slic_conv_wgrad): M < 2^24 output positions, x and dy below 4 GiB - 256 B.
 * Stands in for the same autograd weight gradient of nn.Conv3d (models/resnet.py:11-17) as slic_conv_wgrad. */
size_t slic_conv_wgrad_wino2_workspace_bytes(const SlicConvArgs* args, int splits);
int slic_conv_wino2_tile_table(const SlicConvArgs* args, uint32_t* tile_tab, void* stream);
int slic_conv_wgrad_wino2(const SlicConvArgs* args, const float* dy, int splits, const uint32_t* tile_tab, float* dW,
                          void* workspace, void* stream);
/* Weight gradient of the same layers by the transposed F(4, 3) algorithm, dW[kw] = sum over W-tiles of G^T[(B^T x) . (A dy)]
 * (six multiplies per (kt, kh, c, n) and tile of four outputs instead of twelve); replaces slic_conv_wgrad where variant 30 runs the
 * forward.  args: the forward geometry (src = x, 3 x 3 x 3 / stride 1 / pad 1, Cs % 64 == 0, N % 64 == 0, any Ws: the last tile of a
 * row may be ragged); dy dense [M][N]; tile_tab: (M / Ws) * ceil(Ws / 4) records of 8 bytes written once per geometry by
 * slic_conv_wino_tile_table; `splits` slices of the tiles,
 * reduced in slice order (deterministic); dW in the reference layout [N][C][3][3][3].  workspace: splits x 9 x 6 x Cs x N floats. */
size_t slic_conv_wgrad_wino_workspace_bytes(const SlicConvArgs* args, int splits);
int slic_conv_wino_tile_table(const SlicConvArgs* args, uint32_t* tile_tab, void* stream);
int slic_conv_wgrad_wino(const SlicConvArgs* args, const float* dy, int splits, const uint32_t* tile_tab, float* dW,
                         void* workspace, void* stream);
/* [B, C, S] -> [B, S, Cp] with channels zero-padded to Cp (clip NCDHW -> NDHWC4, datasets/dataset_utils.py:104) */
int slic_ncdhw_to_ndhwc(const float* x, int B, int C, int64_t S, int Cp, float* y, void* stream);
/* [B, C, R, W] -> [B, R, Wp, C] (R = T*H rows): column w lands at w + pad_left, the other columns are zero (Wp >= W + pad_left):
 * the W-run stem operand */
int slic_ncdhw_to_ndhwc_wpad(const float* x, int B, int C, int64_t R, int W, int pad_left, int Wp, float* y, void* stream);

/* Data gradient of the stem convolution with respect to the clip (csrc/stem_dgrad.hip): kernel kt x 7 x 7, stride (st, 2, 2),
 * pad (kt / 2, 3, 3), 1 <= C <= 4 input channels, N % 8 == 0 output channels, kt odd <= 7, st 1 or 2, any T, H, W.
 * dz [B, To, Ho, Wo, N] (NDHWC, To = (T - 1) / st + 1, Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1, 16-byte aligned) ->
 * dx [B, C, T, H, W] (NCDHW, the clip's own layout; every element is written).  Exact fp32, fixed summation order, no atomics.
 * Wp: kt * 16 * N * 16 floats from slic_pack_weight_stem_dgrad — W in the reference layout [N, C, kt, 7, 7] spread over the 4 x 4
 * (h, w) offsets into dz and the C x 2 x 2 (channel, h parity, w parity) columns, zero where a parity class has no tap.
 * Any other shape: non-zero return with slic_last_error set. */
int slic_pack_weight_stem_dgrad(const float* W, int N, int C, int kt, float* Wp, void* stream);
int slic_conv_stem_dgrad(const float* dz, const float* Wp, int B, int C, int T, int H, int W, int N, int kt, int st, float* dx,
                         void* stream);

/* SyncBatchNorm (online_train.py:466-468 -> torch.nn.SyncBatchNorm.convert_sync_batchnorm): the rank-local halves of
 * slic_bn_finalize / slic_bn_bwd*, with the collective left to the caller (torch.distributed over RCCL).
 *   forward : slic_bn_merge_stats -> stats[0..C) = sum, stats[C..2C) = M2 (doubles); the caller writes its sample count to
 *             stats[2C], all-gathers the rows in rank order, and every rank runs slic_bn_finalize_sync on [W][2C+1]
 *             (Chan's merge in rank order; normalisation with the biased variance, running stats with the unbiased one over
 *             the global count).
 *   backward: slic_bn_bwd_sums -> sums[0..C) = sum g, sums[C..2C) = sum g*xhat (doubles, rank-local) + rank-local dgamma/dbeta,
 *             from a dgrad epilogue's slab (partial, R_partial) or, partial == NULL, from dy / out (ReLU mask) / z with the masked
 *             gradient written to g_out; the caller all-reduces `sums`, divides by the global count (ka, kb) and calls
 *             slic_bn_bwd_apply. */
int slic_bn_merge_stats(const float* partial, int R, int rows, int C, int64_t M, double* stats, void* workspace, void* stream);
int slic_bn_finalize_sync(const double* stats_all, int W, int C, float eps, float momentum, const float* gamma,
                          const float* beta, float* mean, float* invstd, float* scale, float* shift,
                          float* running_mean, float* running_var, void* stream);
size_t slic_bn_bwd_sums_workspace_bytes(int64_t M, int C, int R_partial);
int slic_bn_bwd_sums(const float* partial, int R_partial, const float* dy, const float* out, const float* z,
                     const float* mean, const float* invstd, int64_t M, int C, float* g_out, double* sums,
                     float* dgamma, float* dbeta, void* workspace, void* stream);
int slic_bn_bwd_apply(const float* g, const float* z, const float* mean, const float* invstd, const float* gamma,
                      const double* ka, const double* kb, int64_t M, int C, float* dz, void* stream);

/* ------------------------------------------------------------------------------------------
 * BatchNorm3d/1d + ReLU + residual + global average pool (models/resnet.py:34-57,132-133,173,183,
 * 294-299; torch defaults eps = 1e-5, momentum = 0.1).  Activations [M, C] row-major, C % 4 == 0.
 * ---------------------------------------------------------------------------------------- */
/* batch statistics from the conv epilogue's per-workgroup slab partial[R][2][C] = (sum, sum (x - mean_blk)^2)
 * over `rows` rows per workgroup (the last one ragged), merged in workgroup order in double (Chan's formula):
 * mean, invstd = 1/sqrt(biased var + eps), scale = gamma*invstd, shift = beta - mean*scale; running stats
 * (optional pair) get the momentum update with the unbiased variance. */
size_t slic_bn_finalize_workspace_bytes(int R, int C);
int slic_bn_finalize(const float* partial, int R, int rows, int C, int64_t M, float eps, float momentum,
                     const float* gamma, const float* beta, float* mean, float* invstd, float* scale,
                     float* shift, float* running_mean, float* running_var, void* workspace, void* stream);
/* eval mode: scale = gamma/sqrt(running_var+eps), shift = beta - running_mean*scale */
int slic_bn_eval_affine(const float* gamma, const float* beta, const float* running_mean,
                        const float* running_var, float eps, int C, float* scale, float* shift, void* stream);
/* y = relu?(z*scale + shift (+ res)) */
int slic_bn_apply(const float* z, const float* scale, const float* shift, const float* res, int relu,
                  int64_t M, int C, float* y, void* stream);
/* backward of y = relu?(BN(z) (+res)) in train mode: g = dy * (out > 0) when `out` (the saved post-ReLU
 * output) is given, else g = dy; g_out (optional) receives g (it is also the gradient of `res`);
 * dz = gamma*invstd*(g - mean(g) - xhat*mean(g*xhat)); dgamma = sum g*xhat; dbeta = sum g. */
size_t slic_bn_bwd_workspace_bytes(int64_t M, int C, int need_g_buffer);
int slic_bn_bwd_rows_per_partial(void);
int slic_bn_bwd(const float* dy, const float* out, const float* z, const float* mean, const float* invstd,
                const float* gamma, int64_t M, int C, float* g_out, float* dz, float* dgamma, float* dbeta,
                void* workspace, void* stream);
/* The second half of slic_bn_bwd when the producer of g (slic_conv_gemm with args->bwd_partial) already applied the
 * ReLU mask and emitted the R x [2][C] partial sums: merges them in slab order (double), writes dgamma / dbeta and
 * dz = gamma*invstd*(g - mean(g) - xhat*mean(g*xhat)). */
size_t slic_bn_bwd_fused_workspace_bytes(int R, int C);
int slic_bn_bwd_fused(const float* partial, int R, const float* g, const float* z, const float* mean,
                      const float* invstd, const float* gamma, int64_t M, int C, float* dz, float* dgamma,
                      float* dbeta, void* workspace, void* stream);
/* AdaptiveAvgPool3d(1): y[b,c] = mean_s x[b,s,c]; backward dx = dy / S */
int slic_avgpool_fwd(const float* x, int B, int S, int C, float* y, void* stream);
int slic_avgpool_bwd(const float* dy, int B, int S, int C, float* dx, void* stream);
/* the stem's nn.MaxPool3d(kernel_size=3, stride=2, padding=1) (models/resnet.py:123, 262-263; `no_max_pool=False`) on an NDHWC
 * tensor: y [B, To, Ho, Wo, C] with To = (T - 1) / 2 + 1 ...; arg (optional) = the winning input position per output element
 * (first maximum in (t, h, w) order), which the backward gathers from */
int slic_maxpool3d_fwd(const float* x, int B, int T, int H, int W, int C, float* y, int32_t* arg, void* stream);
int slic_maxpool3d_bwd(const float* dy, const int32_t* arg, int B, int T, int H, int W, int C, float* dx, void* stream);
/* shortcut_type 'A' (models/resnet.py:213-222): every stride-th position of x [B, T, H, W, C], channels zero-padded to C_out.
 * The reference concatenates `out.data`, so the branch carries no gradient: there is no backward entry */
int slic_shortcut_a(const float* x, int B, int T, int H, int W, int C, int stride, int C_out, float* y, void* stream);
/* out[c] = sum_m x[m,c] (rows ascending, double accumulator): nn.Linear bias gradient */
int slic_colsum(const float* x, int64_t M, int C, float* out, void* stream);

/* ------------------------------------------------------------------------------------------
 * InfoNCE / NT-Xent (loss/triplet_loss.py:95-116 'noise_contrastive' + pdist :429-437):
 * loss = CE( (1 - (1 - cos(e_i, e_j))) with diag := 0, / T ;  target (n/2 + i) mod n ), mean over n rows.
 * fwd keeps (e_hat, 1/norm, row log-sum-exp) in `workspace` for bwd.  gscale: device scalar upstream
 * gradient (NULL = 1).  D even.
 * ---------------------------------------------------------------------------------------- */
size_t slic_ntxent_workspace_bytes(int n, int D);
int slic_ntxent_fwd(const float* E, int n, int D, int lde, float temperature, float* loss, void* workspace,
                    void* stream);
int slic_ntxent_bwd(const void* workspace, int n, int D, float temperature, const float* gscale, float* dE,
                    int ldd, void* stream);
/* rowwise distance of two [n, D] matrices: 1 - cos (per-norm clamp 1e-8) or ||x - y + 1e-6||_2
 * (models/triplet_net.py:29-33: F.cosine_similarity / F.pairwise_distance) */
int slic_pair_distance(const float* X, const float* Y, int n, int D, int euclidean, float* out, void* stream);
/* its backward: dX, dY [n, D] from g [n] = dL/d dist (the reference's distances are ordinary autograd nodes,
 * models/triplet_net.py:28-32) */
int slic_pair_distance_bwd(const float* X, const float* Y, const float* g, int n, int D, int euclidean, float* dX, float* dY,
                           void* stream);
/* LLC margin term of triplet_train_epoch (online_train.py:317-332): loss = mean_i max(0, (1 - cos(x_i, y_i)) -
 * (1 - cos(x_i, z_i)) + margin)  (MarginRankingLoss with target -1 on the two cosine distances).
 * state: [n][8] floats kept for bwd = {cos(x,y), cos(x,z), |x|, |y|, |z| (each norm clamped at 1e-8), active (1 where the hinge
 * argument is > 0, else 0), two unused}; the euclidean form keeps {d1, d2, -, -, -, active, -, -}; unused slots are not written.
 * rowloss: [n] scratch.  bwd: gradients to all three inputs (exactly 0 for a row whose hinge argument is <= 0). */
int slic_margin_cos_fwd(const float* X, const float* Y, const float* Z, int n, int D, float margin, float* state,
                        float* rowloss, float* loss, void* stream);
int slic_margin_cos_bwd(const float* X, const float* Y, const float* Z, const float* state, int n, int D,
                        const float* gscale, float* dX, float* dY, float* dZ, void* stream);
/* the same margin term on euclidean distances, F.pairwise_distance(x, y) = ||x - y + 1e-6||_2 (LOSS.DIST_METRIC 'euclidean':
 * loss/triplet_loss.py:68-70, 212-214; online_train.py:289-291, 317-319, 345-347); state / rowloss as above */
int slic_margin_euclid_fwd(const float* X, const float* Y, const float* Z, int n, int D, float margin, float* state,
                           float* rowloss, float* loss, void* stream);
int slic_margin_euclid_bwd(const float* X, const float* Y, const float* Z, const float* state, int n, int D,
                           const float* gscale, float* dX, float* dY, float* dZ, void* stream);
/* 'noise_contrastive' with dist_metric 'euclidean' (loss/triplet_loss.py:97-116): logits (1 - ||e_i - e_j||) / T, diagonal 0,
 * target (n / 2 + i) mod n, mean cross-entropy.  dist, wm: [n, n] floats kept for the backward; rowloss: [n] scratch */
int slic_ntxent_euclid_fwd(const float* E, int n, int D, float temperature, float* dist, float* wm, float* rowloss, float* loss,
                           void* stream);
int slic_ntxent_euclid_bwd(const float* E, const float* dist, const float* wm, int n, int D, const float* gscale, float* dE,
                           void* stream);
/* negative selection of NegativeTripletSelector.get_one_one_triplets (loss/triplet_loss.py:311-360) for P (anchor,
 * positive) pairs over the [n, n] distance matrix `dist`: mode 0 random_negative, 1 random_semi_hard, 2 fixed_semi_hard;
 * u[P] uniform in [0,1) stands in for Python's random.choice (unused for mode 2); fallback = hardest easy negative,
 * returned as its position in the negatives list exactly like the reference.  labels: int64 [n], compared as 64-bit.
 * The contract on u is [0, 1) (torch.rand); the rank is floor(u * count) evaluated in float32 (count converted to float, one
 * rounded product), in ascending column order, and a product that rounds up to count is taken as count - 1.  Ties of the
 * arg-max (mode 2) and of the closest negative (fallback) go to the lowest column. */
int slic_triplet_select(const float* dist, const int64_t* labels, int n, const int32_t* anchors,
                        const int32_t* positives, int P, float margin, int mode, const float* u, int32_t* negatives,
                        void* stream);
/* the K (<= 8) negatives per pair of the reference's 'all_semi_hard' branch (loss/triplet_loss.py:158-183, K = 5 there): K distinct rows
 * among the first max(K, #semi-hard) rows of the anchor's negatives list (ascending rows); u[P][K] uniforms in [0, 1) stand in for
 * random.sample (draw t = the floor(u (L - t))-th position not taken yet).  negatives: int32 [P][K].  *status (int32, caller-zeroed) is
 * raised to 1 when an anchor has fewer than K negatives (the reference's topk fails there); such pairs get -1. */
int slic_triplet_select_k(const float* dist, const int64_t* labels, int n, const int32_t* anchors, const int32_t* positives, int P,
                          float margin, int K, const float* u, int32_t* negatives, int32_t* status, void* stream);
/* the same over a rectangular matrix dist[rows][ncols] (MemTripletLoss, loss/triplet_loss.py:9-81, 239-272: rows = the batch,
 * columns = the queue): col_labels int64 [ncols], the pair's anchor row / anchor label / positive COLUMN; mode 3 =
 * 'adapted_hard' (the reference's sampler returns nothing, so every pair takes the hardest-easy fallback). */
int slic_triplet_select_cross(const float* dist, const int64_t* col_labels, int ncols, const int32_t* anchor_rows,
                              const int64_t* anchor_labels, const int32_t* positive_cols, int P, float margin, int mode,
                              const float* u, int32_t* negatives, void* stream);
/* [n, n] distance matrix of the rows of V (loss/triplet_loss.py:429-437 pdist) */
int slic_pdist(const float* V, int n, int D, float eps, int euclidean, float* out, void* stream);
/* [nx, ny] distance matrix between the rows of X and Y (loss/triplet_loss.py:439-447 pdist_v2) */
int slic_pdist2(const float* X, int nx, const float* Y, int ny, int D, float eps, int euclidean, float* out, void* stream);
/* InfoNCE over gathered rows ('all_semi_hard', loss/triplet_loss.py:118-203): X [P, D] anchors, Y [P, NY, D] with row 0 the
 * positive and rows 1..NY-1 the picked negatives (NY <= 8): loss = mean_i -log(e^{cos(x,y0)/T} / sum_j e^{cos(x,yj)/T}).
 * state [P][18] floats = {cos_0 .. cos_7, |y_0| .. |y_7|, |x|, sum_j e^{cos_j/T}} (norms clamped at 1e-8; the slots of j >= NY are
 * not written) is kept for the backward, which returns dX [P, D] and dY [P, NY, D] scaled by *gscale. */
int slic_infonce_rows_fwd(const float* X, const float* Y, int P, int NY, int D, float temperature, float* state,
                          float* rowloss, float* loss, void* stream);
int slic_infonce_rows_bwd(const float* X, const float* Y, const float* state, int P, int NY, int D, float temperature,
                          const float* gscale, float* dX, float* dY, void* stream);

/* ------------------------------------------------------------------------------------------
 * Cosine top-k retrieval (iic_retrieve_clips.py:275-314 topk_retrieval; evaluate.py:208-231,287-307):
 * sklearn cosine_distances + argsort/argpartition on the host become a fused similarity GEMM +
 * streaming top-k; the Nq x Ng matrix is never written.
 * ---------------------------------------------------------------------------------------- */
/* sklearn.preprocessing.normalize(X, 'l2'): out[i,:] = X[i,:] / ||X[i,:]|| (zero rows unchanged); out is dense [N, D] */
int slic_normalize_rows(const float* X, int64_t N, int D, int ldx, float* out, void* stream);
/* for every row of Qn the k nearest rows of Gn by cosine distance clip(1 - q.g, 0, 2), ascending (ties -> lower
 * gallery index).  Qn/Gn: normalised, dense [N, D], D % 8 == 0.  self_mask != 0 skips j == i
 * (np.fill_diagonal(distance_matrix, inf), evaluate.py:221-222).  k <= 88 (SLIC_EINVAL beyond: the per-query lists of the
 * streaming kernels live in LDS).  Two algorithms, identical results: galleries of >= 32768 rows with D <= 512 and k >= 16 go threshold ->
 * collect -> select (a strided sample of the gallery gives every query a score threshold that ~6 k + 100 rows reach; the similarity
 * pass appends the rows that reach it to a candidate buffer — no list kept; one wave per query then sorts out the k best; a query
 * whose candidate count fell outside [k, 2048] is redone by the streaming kernels: exact for any data); everything else, and
 * SLIC_TOPK_COLLECT=0, streams per-(query, gallery slice) k-slot heaps in LDS and merges them (SLIC_TOPK_COLLECT=1: collect for any k). */
size_t slic_cosine_topk_workspace_bytes(int Nq, int Ng, int k);
/* which of the two a call takes and the collect path's sample: out[0] = 1 collect / 0 streaming, out[1] = sample slices, out[2] = rows
 * per sample slice, out[3] = M (the threshold is the M-th best of the pooled sample), out[4] = gallery row step of the sample, out[5] = candidate
 * slots per query.  Introspection for tests and bench lines; no device work. */
int slic_cosine_topk_plan(int Nq, int Ng, int D, int k, int* out /* [6] */);
int slic_cosine_topk(const float* Qn, int Nq, const float* Gn, int Ng, int D, int k, int self_mask,
                     int32_t* out_idx, float* out_dist, void* workspace, void* stream);
/* The same search with the similarity GEMM on the bf16 MFMA as a CANDIDATE pass; the result is exact.  Rows rounded to bf16 give a coarse
 * score c with |c - s| <= slic_cosine_topk_bf16_eps() (0.008: proven for L2-normalised rows, D <= 512, fp32 accumulation — DESIGN.md) of
 * the fp32 score s.  Every row with c >= tau_q - eps (tau_q: the collect path's fp32 sample threshold) is a candidate; with c_k the k-th
 * best coarse score, a row of the true top-k has c >= c_k - 2 eps, so those candidates are rescored from the fp32 rows and the k best of
 * them are the global top-k (distance ascending, ties -> lower index, distance = clip(1 - s, 0, 2)).  A query with fewer than k
 * candidates, or more than its slots, is redone by the fp32 streaming kernels: the result is exact for any data.
 * Limits as slic_cosine_topk.  The bf16 pass runs where slic_cosine_topk_bf16_plan says so: inside the collect path's domain (Ng >= 32768,
 * D <= 512) and where it measured faster than the fp32 path (Nq * Ng >= 1e9, D >= 128, k <= 50: profiles/topk_bf16.txt) — SLIC_TOPK_BF16=1: anywhere in that domain, for any
 * k; SLIC_TOPK_BF16=0: nowhere.  Elsewhere the call IS slic_cosine_topk (and the workspace size is that call's).
 *   plan   out[0] = 1 bf16 pass / 0 fp32 search, out[1] = candidate slots per query, out[2] = columns of a bf16 row (D rounded up to 16),
 *          out[3] = queries per workgroup, out[4] = sampled gallery rows, out[5] = M (tau_q is the M-th best of the sample).  No device work.
 *   stats  NULL or a DEVICE array of 3: {queries redone by the fp32 kernels, queries whose candidates overflowed their slots, candidates
 *          of all queries (an overflowed query counts its slots)}; all 0 when the call took the fp32 search. */
size_t slic_cosine_topk_bf16_workspace_bytes(int Nq, int Ng, int D, int k);
int slic_cosine_topk_bf16_plan(int Nq, int Ng, int D, int k, int* out /* [6] */);
int slic_cosine_topk_bf16(const float* Qn, int Nq, const float* Gn, int Ng, int D, int k, int self_mask,
                          int32_t* out_idx, float* out_dist, int32_t* stats, void* workspace, void* stream);
float slic_cosine_topk_bf16_eps(void);
/* merge W per-GPU result lists ([W, Nq, k] distances ascending + GLOBAL gallery indices, -1 = empty slot) into the
 * k nearest per query (distance ascending, ties -> lower index): the step after the all-gather when the gallery is
 * sharded by rows across GPUs */
int slic_topk_merge_lists(const float* pdist, const int32_t* pidx, int W, int Nq, int k, int32_t* out_idx,
                          float* out_dist, void* stream);
/* Euclidean top-k retrieval (LOSS.DIST_METRIC 'euclidean': validation.py:81,130, evaluate.py:367): for every row of Q the k nearest
 * rows of G by |q - g|_2, ascending (ties -> lower gallery index); self_mask as above.  Q [Nq, D] (row stride ldq), G [Ng, D] (ldg): raw
 * rows, any D; the library centres both on G's column mean and pads D to a multiple of 8 in its workspace.  The cosine path's kernels rank
 * the k + 8 (at most 88, at most Ng) best rows by q.g - |g|^2 / 2, then the distances of those rows are recomputed directly from the raw
 * rows in float64 and the k nearest are kept: exact duplicates come back at 0.  Limits as slic_cosine_topk (1 <= k <= min(88, Ng);
 * SLIC_EINVAL beyond).  The path choice is slic_cosine_topk_plan(Nq, Ng, D rounded up to 8, that list length), SLIC_TOPK_COLLECT alike. */
size_t slic_euclidean_topk_workspace_bytes(int Nq, int Ng, int D, int k);
int slic_euclidean_topk(const float* Q, int Nq, int ldq, const float* G, int Ng, int ldg, int D, int k, int self_mask,
                        int32_t* out_idx, float* out_dist, void* workspace, void* stream);
/* euclidean_distances(X, Y) as a dense [Nx, Ny] matrix (evaluate.py:216; validation-size inputs) */
int slic_pairwise_euclidean(const float* X, int Nx, const float* Y, int Ny, int D, float* out, void* stream);

/* ------------------------------------------------------------------------------------------
 * The validation pass (validation.py:12-151): the per-batch arithmetic after the encoder.
 * ------------------------------------------------------------------------------------------ */
/* validation.py:59-71 as ONE launch on the three [B, D] embedding matrices of a batch: dist_a[b] = d(ex[b], ey[b]) and
 * dist_b[b] = d(ex[b], ez[b]) with the arithmetic — and the bits — of slic_pair_distance (either may be NULL);
 * rec[0] = mean_b max(0, dist_a[b] - dist_b[b] + margin)   (MarginRankingLoss(margin)(dist_a, dist_b, -1), mean reduction),
 * rec[1] = #{b : dist_b[b] - dist_a[b] > 0} / B            (accuracy, models/model_utils.py:232-235), rec[2] = B: one row of the
 * epoch record.  One workgroup walks the rows; the sums have a fixed order, so the result does not depend on scheduling.
 * SLIC_EINVAL for B < 1 or D < 1. */
int slic_triplet_val_batch(const float* ex, const float* ey, const float* ez, int B, int D, int euclid, float margin, float* dist_a,
                           float* dist_b, float* rec, void* stream);
/* get_topk_acc's double loop (evaluate.py:296-305) on a device-resident [Nq, k] index table (slic_cosine_topk / slic_euclidean_topk /
 * slic_topk_merge_lists): first_hit[q] (NULL = not wanted) = the first column j with g_labels[idx[q, j]] == q_labels[q], k if none;
 * hits[i] = #{q : first_hit[q] < top_ks[i]} — written, not accumulated.  Entries < 0 (merge padding) or >= Ng never hit.  top_ks is
 * a HOST array of n_ks <= 8 ascending values in 1 .. k; everything else lives on the device.  Integer counts: exact. */
int slic_topk_label_hits(const int32_t* idx, int Nq, int k, const int64_t* q_labels, const int64_t* g_labels, int Ng,
                         const int32_t* top_ks, int n_ks, int32_t* first_hit, int32_t* hits, void* stream);

/* ------------------------------------------------------------------------------------------
 * DBSCAN, cosine metric (clustering/cluster_masks.py:55-61 -> sklearn.cluster.DBSCAN(eps, min_samples, metric='cosine')):
 * labels = DBSCAN(eps, min_samples, metric='cosine').fit(X).labels_ of sklearn 1.7 (sklearn/cluster/_dbscan.py:410-438,
 * _dbscan_inner.pyx).  Rules:
 *   1. j is in N(i) iff d(i, j) <= eps, d = clip(1 - (x_i . x_j) * inv_i * inv_j, 0, 2) for j != i: the dot of the raw fp32 rows and
 *      the inverse norms inv = 1 / ||x|| (0 for a zero row) all in float64; d(i, i) = 0 (sklearn's radius search of X against
 *      itself zeroes the diagonal), so a zero row is its own neighbour and at distance 1 from every other row.  Every
 *      pair is decided this way (fp32 similarity GEMM, float64 recheck of the scores within a proven error band of 1 - eps), so the
 *      relation is symmetric and the same in every pass.  sklearn decides in float32: the two agree except within ~1e-6 of eps.
 *   2. i is core iff |N(i)| >= min_samples (i itself counts when it is its own neighbour).
 *   3. clusters = connected components of the core rows under the neighbour relation, numbered 0, 1, ... by their smallest row.
 *   4. a non-core row with a core neighbour takes the smallest cluster number among its core neighbours; other rows are noise, -1.
 * X: [N, D] fp32, row stride ldx >= D (elements), 1 <= D <= 512.  Outputs (device): labels int32 [N], is_core uint8 [N] (0 / 1),
 * counts int32 [N] = |N(i)| (NULL: not returned), *n_clusters int32.  All are integers fixed by the rules: two runs are bit-equal.
 * SLIC_EINVAL for eps < 0, min_samples < 1, D outside [1, 512], N < 1, or rows beyond int32 indices / a 4 GiB padded copy (no wrap).
 * The N x N matrix is never written; the workspace is O(N * Dp + N) with Dp = D rounded up to 8. */
size_t slic_dbscan_cosine_workspace_bytes(int64_t N, int D);       /* 0 for sizes slic_dbscan_cosine rejects */
int slic_dbscan_cosine(const float* X, int64_t N, int ldx, int D, double eps, int min_samples, int32_t* labels, uint8_t* is_core,
                       int32_t* counts, int32_t* n_clusters, void* workspace, void* stream);
/* after a slic_dbscan_cosine call with this workspace (synchronises the stream): out_host[0] = pairs rechecked in float64,
 * [1] link-pass tiles skipped (all rows in one component already), [2] core rows, [3] border candidates, [4..9] ms of the passes
 * prep / count / compact / link / number / border when SLIC_DBSCAN_TIMING=1 was set at the call (else -1).  Measurement only. */
int slic_dbscan_cosine_stats(const void* workspace, double* out_host /* [10] */, void* stream);

/* ------------------------------------------------------------------------------------------
 * OPTICS, cosine metric, cluster_method='dbscan' (clustering/cluster_masks.py:88-89 -> sklearn.cluster.OPTICS(min_samples, max_eps,
 * metric='cosine', cluster_method='dbscan', eps=None)): labels_, core_distances_, reachability_, predecessor_ and ordering_ of sklearn
 * 1.7 (sklearn/cluster/_optics.py: compute_optics_graph, _set_reach_dist, cluster_optics_dbscan).  Rules:
 *   1. Neighbour relation.  j is in N(i) iff d64(i, j) <= max_eps: exactly slic_dbscan_cosine's rule 1 (an fp32 score, a float64 recheck
 *      from the raw rows inside a proven band around 1 - max_eps; d(i, i) = 0; a zero row is at distance 1 from every other row).  The
 *      relation is symmetric and the same in every pass, the walk included.
 *   2. Core rows.  i is core iff |N(i)| >= min_samples, the row itself counted.
 *   3. Core distances.  d32(i, j) is ONE device function of the normalised zero-padded rows Xn_i, Xn_j: clip(1 - dot, 0, 2), the fp32
 *      dot summed in a fixed order (lane l of a wave takes elements l, l + 64, ... by fmaf, then an xor butterfly), symmetric in its
 *      arguments, d32(i, i) = 0.  core_distances_[i] = the min_samples-th smallest of {0} u {d32(i, j), j != i} for a core row, +inf
 *      for a non-core row.  It is evaluated as d32(i, j_k), j_k the last entry of slic_cosine_topk's self-masked list of
 *      min_samples - 1 rows for row i on Xn, so that the relax step below gets max(d32(p, j_k), cd[p]) == cd[p] bit for bit: the
 *      structural ties of OPTICS are exact ties.  The core flag is decided in float64 and the value is fp32: a core row's value may
 *      exceed max_eps by an fp32 rounding, where sklearn would write inf.
 *   4. Walk.  reachability_ = +inf, predecessor_ = -1.  N times: take the unprocessed row p with the smallest reachability (an exact
 *      tie goes to the lowest row index; when all are +inf that is the lowest unprocessed row) and append it to ordering_; if p is
 *      core, every unprocessed j in N(p) gets r = max(d32(p, j), cd[p]) and, if r < reachability_[j] (strict), reachability_[j] = r,
 *      predecessor_[j] = p.  (sklearn rounds r to 15 decimals in float64: nothing to reproduce in fp32.)
 *   5. Labels (eps = max_eps).  Clusters = the connected components of the core rows under rule 1, numbered 0, 1, ... by their
 *      smallest row.  A non-core row b with a core neighbour looks at the clusters of those neighbours, takes the one whose smallest
 *      core row s is smallest and keeps it only if s < b; otherwise, and without a core neighbour, it is noise, -1.  (DBSCAN's rule 4
 *      has no s < b test: the walk reaches such a row as a start of its own before any core of its clusters.)  The labels come from
 *      parallel passes, not from the walk; cutting the walk's reachability plot at max_eps gives the same labels.
 *   6. All outputs are fixed by rules 1-5: two runs are bit-equal.
 * The walk runs every cluster at once (a cluster's walk touches its own rows only; ordering_ interleaves the clusters' blocks and the
 * noise rows by start time), so the dependent steps are the largest cluster's rows, not N.
 * X: [N, D] fp32, row stride ldx >= D.  Outputs (device): labels int32 [N], is_core uint8 [N] (NULL: not returned), core_dist fp32 [N],
 * reachability fp32 [N], predecessor int32 [N], ordering int32 [N], *n_clusters int32 (NULL: not returned).  reachability, predecessor
 * and ordering are given together or all NULL: NULL skips the walk (labels only; core_dist may then be NULL too, which also skips the
 * core-distance search).  With the walk the call synchronises the stream once (the cluster sizes size its launches).
 * SLIC_EINVAL for min_samples < 2, min_samples > N, min_samples > 89 (the search's list length), max_eps < 0 or not finite, D outside
 * [1, 512], N < 1 or rows beyond slic_dbscan_cosine's limits.  No N x N matrix and no neighbour lists are written; the workspace is
 * O(N * Dp + N * min_samples) (the label passes' 2 N Dp floats, the search's lists). */
size_t slic_optics_cosine_workspace_bytes(int64_t N, int D, int min_samples);       /* 0 for arguments slic_optics_cosine rejects */
int slic_optics_cosine(const float* X, int64_t N, int ldx, int D, double max_eps, int min_samples, int32_t* labels, uint8_t* is_core,
                       float* core_dist, float* reachability, int32_t* predecessor, int32_t* ordering, int32_t* n_clusters,
                       void* workspace, void* stream);
/* after a slic_optics_cosine call with this workspace (synchronises the stream): out_host[0] = pairs rechecked in float64 by the label
 * passes, [1] by the walk, [2] core rows, [3] clusters, [4] rows of the largest cluster = the walk's dependent steps, [5] those
 * steps again as the host counted them, [6] launches of the walk, [7] clusters walked by the host loop (more rows than one workgroup
 * keeps in LDS; the rest are walked by one workgroup each), [8..13] ms of the label passes prep / count / compact / link / number /
 * border, [14] ms of the core distances, [15] ms of the walk when SLIC_OPTICS_TIMING=1 was set at the call (else -1; [3..7] are -1 / 0
 * and [14], [15] -1 for the parts a labels-only call skipped).  Measurement only. */
int slic_optics_cosine_stats(const void* workspace, double* out_host /* [16] */, void* stream);

/* ------------------------------------------------------------------------------------------
 * HDBSCAN, cosine metric (sklearn.cluster.HDBSCAN(min_cluster_size, min_samples, metric='cosine') of sklearn 1.7: density clusters with
 * noise and no radius to tune).  The device does what is O(N^2 D): core distances and the minimum spanning tree of the mutual
 * reachability weights, by Boruvka rounds; the caller keeps the components between the rounds and turns the N - 1 edges into labels
 * (clustering/hdbscan.py).  Rules:
 *   1. d(i, j) = clip(1 - x^_i . x^_j, 0, 2) on the L2-normalised rows.  A zero row is at distance 1 from every other row, as in
 *      slic_dbscan_cosine's rule 1.  d(i, i) = 0.
 *   2. core(i) = the min_samples-th smallest entry of row i of d INCLUDING the diagonal zero: sklearn's
 *      np.partition(D, min_samples - 1)[:, min_samples - 1] (min_samples = 1: core = 0).
 *   3. w(i, j) = max(d(i, j), core(i), core(j)).
 *   4. The tree is the minimum spanning tree of w under the total order (w, min(i, j), max(i, j)), which makes it unique.
 *   5. From the tree, on the host, by the HDBSCAN definition: the single-linkage tree of the edges sorted in that order, the condensed
 *      tree with min_cluster_size and lambda = 1 / height, stability, 'eom' or 'leaf' selection with allow_single_cluster,
 *      cluster_selection_epsilon, labels_ (noise = -1) and probabilities_.
 *   6. Clusters are numbered 0, 1, ... by their smallest row (sklearn numbers by condensed-tree id: the partitions are equal).
 * Arithmetic.  The searches see fp32: the rows are normalised with a float64 inverse norm and rounded to fp32 (zero-padded to Dp = D
 * rounded up to 8), a score is the fp32 MFMA dot of two such rows, |score - exact| <= (Dp + 2) 2^-24.  Every value that is REPORTED
 * is float64 of the raw fp32 rows: the dot of the pair (lower row first; lane l of a wave takes elements l, l + 64, ... by fma, then an
 * xor butterfly: one fixed order, the same from either end of the pair) times the float64 inverse norms.
 *   slic_hdbscan_core          prep, then slic_cosine_topk of the rows against themselves (self_mask = 0, k = min_samples: the row itself is
 *                              in its list, rule 2's diagonal) and core_dist[i] (device, float64 [N]) = the float64 distance to the
 *                              list's last row (0 when that is the row itself).  The normalised rows and an fp32 copy of core_dist stay
 *                              in the workspace: the state of the two calls below.
 *   slic_hdbscan_round         one Boruvka round, the hot path: a streamed rows x rows^T pass (the MFMA row-tile ring) that finds for every
 *                              row i min_j w32(i, j) over the rows j with comp[j] != comp[i], w32 = max(fp32 d, fp32 core(i), fp32
 *                              core(j)), a tie going to the smaller j; then for every component c in [0, C) its least (w32, lo, hi)
 *                              over its rows, (lo, hi) = (min, max) of (i, j): out_i[c] = lo, out_j[c] = hi, out_w[c] = w32 (device
 *                              arrays of C; -1, -1, +inf for a component with no foreign row, i.e. C == 1).  comp: device int32 [N]
 *                              with values in [0, C) (a row with another value proposes nothing).  row_best: NULL, or a device array
 *                              of N that receives (bits of w32 << 32) | j per row (all ones: no foreign row).  All reductions are
 *                              64-bit integer atomicMin: order-independent.  fp32 scores seen from the two ends of a pair may differ
 *                              in the last bit, so the candidates of a round may close a cycle: the caller applies them through
 *                              union-find in the order (float64 w, lo, hi) and drops an edge whose ends are already connected; every
 *                              component still proposes an edge that leaves it, so the rounds end with a spanning tree after at most
 *                              ceil(log2 N) of them.  With exact weights every candidate is an edge of rule 4's tree.
 *   slic_hdbscan_edge_weights  out[e] (device, float64 [M]) = rule 3's w in float64 for pairs[e] = (i, j) (device int32 [M, 2]), one wave
 *                              per pair; NaN for a pair outside the rows.  core_dist: slic_hdbscan_core's output.
 *   slic_hdbscan_stats         out_host[0] = rounds since the last slic_hdbscan_core, [1] rows searched by the last round, [2] ms of the
 *                              core call, [3] ms of all rounds, [4] of the last round, [5] of its streamed pass alone when
 *                              SLIC_HDBSCAN_TIMING=1 was set at the calls (else -1; the timed calls synchronise).  Measurement only.
 * No float atomics: two runs are bit-equal.  The N x N matrix is never written; the workspace is O(N * Dp + N * min_samples).
 * X: [N, D] fp32, row stride ldx >= D.  SLIC_EINVAL for N < 2, D outside [1, 512], min_samples outside [1, min(N, 88)] (the search's list
 * length), rows beyond slic_dbscan_cosine's limits (int32 row indices, < 4 GiB padded), C outside [1, N].  N, D and min_samples of the
 * later calls are those of the slic_hdbscan_core call that filled the workspace. */
size_t slic_hdbscan_workspace_bytes(int64_t N, int D, int min_samples);       /* 0 for arguments slic_hdbscan_core rejects */
int slic_hdbscan_core(const float* X, int64_t N, int ldx, int D, int min_samples, double* core_dist, void* workspace, void* stream);
int slic_hdbscan_round(void* workspace, int64_t N, int D, int min_samples, const int32_t* comp, int C, int32_t* out_i, int32_t* out_j,
                       float* out_w, uint64_t* row_best, void* stream);
int slic_hdbscan_edge_weights(const float* X, int64_t N, int ldx, int D, int min_samples, const double* core_dist, const int32_t* pairs,
                              int64_t M, double* out, void* workspace, void* stream);
int slic_hdbscan_stats(double* out_host /* [6] */);

/* ------------------------------------------------------------------------------------------
 * Average-linkage agglomerative clustering, cosine metric, cut by a distance threshold (clustering/cluster_masks.py:49-54 ->
 * sklearn.cluster.AgglomerativeClustering(n_clusters=None, linkage='average', distance_threshold=t, affinity='cosine')).
 * The rows are L2-normalised (slic_normalize_rows) and zero-padded to Dp = D rounded up to 8.  A cluster is the sum S of its unit rows and
 * their number n; d(A, B) = clip(1 - (S_A / n_A) . (S_B / n_B), 0, 2) in fp32, as slic_cosine_topk computes it on the means: the average
 * of all pairwise cosine distances between A and B.  State lives in the caller's workspace between the calls:
 *   slic_agglo_start          every row a live, "stale" cluster.  *bad_rows_host = rows of zero norm or with a non-finite value: an argument
 *                             error the caller reports (nothing else may be called on that workspace then).  Synchronises the stream.
 *   slic_agglo_round          A = live clusters, Q = stale live clusters (the host knows both: N, N after the start, then the record's).
 *                             Every stale cluster searches the A means for its nearest OTHER cluster nn (ties -> lower id) at distance nd;
 *                             every pair a < b with nn[a] == b, nn[b] == a and nd[a] < threshold merges: S[a] += S[b], n[a] += n[b], b dies,
 *                             parent[b] = a.  Then a live cluster is stale when it merged or its nn merged or died (average linkage is
 *                             reducible: any other cached nn is still a nearest cluster).  record_host (SLIC_AGGLO_RECORD int64):
 *                             [0] pairs merged, [1] live clusters, [2] stale clusters after the round, [3] (bits of nd << 32) | id of the
 *                             live cluster with the smallest (nd, id) at the start of the merge step, [4] nanoseconds the search took on
 *                             the device when SLIC_AGGLO_TIMING=1 was set at the call (else -1; measurement only).  One device-to-host
 *                             copy and one synchronisation per round.  topk_workspace: slic_cosine_topk_workspace_bytes(Q, A, 2) bytes.
 *   slic_agglo_merge_closest  after a round that merged nothing: merges the record's closest cluster [3] with its nn (the lower id
 *                             survives) and marks stale as a round does; record_host [0] = 1 (0 if there was no such pair), [1], [2] as above.
 *   slic_agglo_labels         labels[i] (device, int32 [N]) = the rank of i's cluster among the live clusters in ascending order of their
 *                             smallest member: 0 .. C-1 in order of first appearance.  The state is left usable.
 * No floating-point atomics: one wave owns a merging pair and every lane its own columns, so two runs give the same bits.
 * Limits: 1 <= N <= SLIC_AGGLO_MAX_N, 1 <= D <= 512, N * Dp * 4 < 4 GiB; SLIC_EINVAL beyond.  The workspace is 3 N Dp floats + O(N). */
#define SLIC_AGGLO_MAX_N ((int64_t)1 << 24)
#define SLIC_AGGLO_RECORD 5
size_t slic_agglo_workspace_bytes(int64_t N, int D);               /* 0 for sizes slic_agglo_start rejects */
int slic_agglo_start(const float* X, int64_t N, int ldx, int D, void* workspace, int32_t* bad_rows_host, void* stream);
int slic_agglo_round(void* workspace, int64_t N, int D, int A, int Q, float threshold, void* topk_workspace, int64_t* record_host,
                     void* stream);
int slic_agglo_merge_closest(void* workspace, int64_t N, int D, int64_t* record_host, void* stream);
int slic_agglo_labels(void* workspace, int64_t N, int D, int32_t* labels, void* stream);

/* ------------------------------------------------------------------------------------------
 * Cluster-quality metrics of the cluster step (online_train.py:633-639 -> sklearn.metrics.normalized_mutual_info_score and
 * adjusted_mutual_info_score, both with average_method='arithmetic'): one call, one fp64 record.  The rules are sklearn 1.7.2's
 * (sklearn/metrics/cluster/_supervised.py:819-924, :1022-1062, :1146-1174, :1281-1314, _expected_mutual_info_fast.pyx):
 *   1. classes / clusters = the distinct values of labels_true / labels_pred (np.unique: any int32 value, -1 like any other, gaps
 *      allowed), numbered in ascending order of value; R = n_classes, C = n_clusters.  n[i][j] = the contingency table, a[i] and
 *      b[j] its row and column sums (integers: exact in any order).
 *   2. MI = max(0, sum over the cells n > 0 of t), t = (n/N) * (log n - log N) + (n/N) * (-log(a*b) + log N + log N), a term with
 *      |t| < 2^-52 counted as 0; MI = 0 when R == 1 or C == 1.
 *   3. H(x) = -sum_i (x_i / N) * (log x_i - log N); 0 for a single class.
 *   4. EMI = sum over i, j and n = max(1, a_i + b_j - N) .. min(a_i, b_j) of (n/N) * (log N + log n - log a_i - log b_j) * exp(g), g = the
 *      log of the hypergeometric weight, sklearn's L(a) + L(b) + L(N-a) + L(N-b) - L(n) - L(N) - L(a-n) - L(b-n) - L(N-a-b+n) with
 *      L(x) = lgamma(x + 1).  Taken literally its terms are ~N log N (2.7e6 at N = 240 000, one ulp = 4.7e-10) and cancel to ~10, so
 *      the last bit of lgamma moves EMI by 1e-10.  The same g in exact arithmetic, with L(N) - L(N - x) = x log N + T(x),
 *      T(x) = sum_{k < x} log1p(-k / N), has no term beyond ~(a + b) log N:
 *          g = ((((L(a) + L(b)) - L(n)) - L(a-n)) - L(b-n)) - n * log N) + ((T(a+b-n) - T(a)) - T(b))      added in this order,
 *      L and T from tables of N + 1 doubles built once per call (T by a fixed-order scan); EMI = 0 when R == 1 or C == 1.
 *   5. NMI = 1 when R == C == 1; else 0 when MI == 0; else MI / ((H_true + H_pred) / 2).
 *   6. AMI = 1 when R == C == 1; else 0 when R == 1 or C == 1; else num / den with num = MI - EMI, den = (H_true + H_pred) / 2 - EMI,
 *      each pushed away from 0 to at least 2^-52 in magnitude, keeping its sign (>= 0 counts as positive).
 * Every fp64 sum has a fixed order: cell (or class) p belongs to thread p mod (1024 * 256) of a 1024 x 256 grid, a thread adds its
 * terms in ascending p (the n of one cell in ascending n first), a workgroup folds its 256 values by halving (v[t] += v[t + s], s = 128
 * .. 1), and one workgroup folds the 1024 partial sums (thread t adds partials t, t + 256, t + 512, t + 768, then the same halving).
 * Two runs on the same labels give the same bits.
 * labels_true, labels_pred: int32 [N] on the device, unit stride.  record (device, SLIC_METRICS_RECORD doubles): MI, H_true, H_pred, EMI,
 * NMI, AMI, n_classes, n_clusters, status.  status 0: the record is valid; 1: R * C exceeds max_cells, nothing else was computed
 * (the other slots hold 0 except the two counts) and the table was not touched.
 * Limits: 1 <= N <= SLIC_METRICS_MAX_N; the dense R x C int32 table lives in the workspace, which the caller sizes with max_cells,
 * 1 <= max_cells <= SLIC_METRICS_MAX_CELLS (2^26 cells, 256 MiB: admits 400 x 65536 and 1024 x 65536).  SLIC_EINVAL beyond.  The
 * workspace is about 61 N + 4 max_cells bytes, sized by the caller's bound and not by the data (the class counts are found on the
 * device); the table is cleared and read over R * C cells only.
 * Cost beyond the sizes the cluster step has (N <= 240 000, measured): each of the 16 radix passes ends in a scan of N / 4 ints by ONE
 * workgroup, and an EMI cell is walked by one thread, so both grow serially: at N = 2^24 a scan covers 4M elements on one compute
 * unit, and two classes of N / 2 labels make one thread walk N / 2 terms.  Correct at every admitted size; tuned for N ~ 10^5. */
#define SLIC_METRICS_MAX_N ((int64_t)1 << 24)
#define SLIC_METRICS_MAX_CELLS ((int64_t)1 << 26)
#define SLIC_METRICS_RECORD 9
size_t slic_cluster_metrics_workspace_bytes(int64_t N, int64_t max_cells);       /* 0 for sizes slic_cluster_metrics rejects */
int slic_cluster_metrics(const int32_t* labels_true, const int32_t* labels_pred, int64_t N, int64_t max_cells, double* record,
                         void* workspace, void* stream);

/* Silhouette coefficient (sklearn.metrics.silhouette_samples / silhouette_score) of rows X [N, D] fp32 (row stride ldx elements, any
 * alignment) under int32 labels [N] (any values; unit stride), for the two metrics whose sum of distances to a cluster follows from
 * the cluster's row sum, so that no N x N and no N x K array is built:
 *   SLIC_SILHOUETTE_COSINE        d(i, j) = 1 - x^_i . x^_j, x^ = x / |x| (a zero row stays zero, as slic_normalize_rows)
 *   SLIC_SILHOUETTE_SQEUCLIDEAN   d(i, j) = |x_i - x_j|^2
 * Clusters get dense ids 0 .. K - 1 by ascending label value.  Per cluster the operand rows (x^ resp. x, fp32) are summed in float64
 * in ascending row order, divided by |C| and rounded once to fp32; |x|^2 is summed in float64 (k ascending), Q_C / |C| likewise.  The
 * mean distance of row i to cluster C is then, in fp32 with every product-sum an fmaf and the dot product a k-ascending fmaf chain
 * from +0 (v_mfma_f32_32x32x2_f32),
 *   cosine: max(1 - x^_i . m_C, 0)        sqeuclidean: max(fmaf(-2, x_i . m_C, |x_i|^2 + Q_C / |C|), 0)
 * b = the smallest over the OTHER clusters (strict '<': the first dense id wins), a = max(fmaf(|C|, d_own, -self), 0) / (|C| - 1)
 * with self = 1 - x^_i . x^_i as computed (cosine) resp. 0, s = (b - a) / max(a, b); s = 0 where max(a, b) == 0 and, with a = 0, for
 * the row of a singleton cluster.  The mean of s over the scored rows and over each cluster is taken in float64 in a fixed order
 * (strided partial sums, folded by halving): two calls on the same input give the same bits; no floating-point atomics.
 * has_ignore != 0: rows labelled ignore_label take no part in any quantity; their s, a, b are NaN, their `nearest` is ignore_label.
 * Outputs (device; each of out_s, out_a, out_b [N] fp32, out_nearest [N] int32 (the nearest other cluster's ORIGINAL label),
 * cluster_mean [Kmax] float64 and cluster_label [Kmax] int32 may be NULL): cluster_mean[j] / cluster_label[j] describe the j-th scored
 * cluster by ascending label, slots past K hold NaN / 0.  record (SLIC_SILHOUETTE_RECORD doubles): mean s, K, rows scored, status.
 * status 0: valid.  SLIC_SILHOUETTE_UNDEFINED: K outside 2 .. rows scored - 1.  SLIC_SILHOUETTE_TOO_MANY: a valid K above Kmax.
 * With a status every float output is NaN and nearest is 0; nothing faults and the call never synchronises with the host.
 * Limits: 3 <= N <= SLIC_SILHOUETTE_MAX_N, 1 <= D <= SLIC_SILHOUETTE_MAX_D (padded to D % 8 == 0 inside), 2 <= Kmax <= N - 1;
 * SLIC_EINVAL beyond.  The workspace (about 4 N (D + 40) + 4 Kmax D bytes) is sized by Kmax, not by the data. */
#define SLIC_SILHOUETTE_COSINE 0
#define SLIC_SILHOUETTE_SQEUCLIDEAN 1
#define SLIC_SILHOUETTE_MAX_N ((int64_t)1 << 24)
#define SLIC_SILHOUETTE_MAX_D 512
#define SLIC_SILHOUETTE_RECORD 4
#define SLIC_SILHOUETTE_UNDEFINED 1
#define SLIC_SILHOUETTE_TOO_MANY 2
size_t slic_silhouette_workspace_bytes(int64_t N, int D, int64_t Kmax);          /* 0 for sizes slic_silhouette rejects */
int slic_silhouette(const float* X, int64_t N, int D, int64_t ldx, const int32_t* labels, int metric, int has_ignore,
                    int32_t ignore_label, int64_t Kmax, float* out_s, float* out_a, float* out_b, int32_t* out_nearest,
                    double* record, double* cluster_mean, int32_t* cluster_label, void* workspace, void* stream);

/* Pair statistics: the distribution of the pairwise cosine distances of rows X [Nx, D] fp32 (row stride ldx elements), split into
 * the pairs whose rows share a label (group 1, "same") and all other pairs (group 0, "diff"), in one streamed pass over the
 * 128 x 128 tiles of the similarity matrix (the walk of slic_dbscan_cosine's count pass); the matrix is never written.
 *   Y == NULL: X against itself, every pair i < j exactly once, a row never with itself (Ny, ldy, ly are not read).
 *   Y != NULL: every pair (q, g) of a row of X and a row of Y [Ny, D] (row stride ldy).
 * Rules:
 *   1. Operands.  inv_i = 1 / ||x_i|| in float64 (k ascending; 0 for a zero row); the operand row is fp32(x_i * inv_i), zero-padded
 *      to D % 8 == 0: slic_dbscan_cosine's preparation, shared in code.  A zero row is therefore at d = 1 from every row, as in
 *      slic_cosine_topk.
 *   2. Score.  s = the fp32 dot product of two operand rows (v_mfma_f32_32x32x2_f32, the MFMA ring's k order);
 *      d = fminf(fmaxf(1.0f - s, 0.0f), 2.0f).
 *   3. Bin.  bin = min(bins - 1, (int)(d * (bins / 2))); bins is a power of two in 8 .. SLIC_PAIR_STATS_MAX_BINS, so the product is
 *      exact: bin b holds b * 2 / bins <= d < (b + 1) * 2 / bins, and d = 2 falls into the last bin.
 *   4. Group.  1 iff both rows carry a label (lx and, with Y, ly are not NULL; int32, unit stride) and the labels are equal, else 0.
 *      Without labels every pair is in group 0.  has_ignore != 0: a row labelled ignore_label takes part in no pair.
 * Outputs (device): hist uint64 [2][bins], hist[g][bin] = pairs of group g in the bin; record (SLIC_PAIR_STATS_RECORD doubles):
 *   n_diff, n_same, sum d (diff, same), sum d^2 (diff, same), sum e (diff, same), status (0),   e = expf(-tt * d), tt = (float)(2 t)
 * (|x^_i - x^_j|^2 = 2 d, so log(sum e / n) is the uniformity of Wang & Isola at temperature t).  d^2 is the float64 square of d.
 * The counts come by integer atomics.  The float64 sums use no floating-point atomic: a lane adds its scores in the tile walk's
 * order, a workgroup folds its lanes by halving, the workgroups' partial sums lie in the workspace and one workgroup adds them in a
 * fixed order: two calls on the same input give the same bits in hist and record.  The call never synchronises with the host.
 * Limits: 1 <= Nx, Ny <= SLIC_PAIR_STATS_MAX_N (Nx = 1 in the self form is valid and counts nothing), 1 <= D <= 512, the padded
 * rows of one side below 4 GiB, 0 < t <= 1e30, row strides in D .. 2^31 - 1; SLIC_EINVAL beyond.  The workspace query takes Ny = 0
 * for the self form; the workspace holds the operand rows, 4 N Dp bytes per side, and 48 bytes per 128 x 2048 block of pairs. */
#define SLIC_PAIR_STATS_MAX_N ((int64_t)1 << 20)
#define SLIC_PAIR_STATS_MAX_BINS 4096
#define SLIC_PAIR_STATS_RECORD 9
size_t slic_pair_stats_workspace_bytes(int64_t Nx, int64_t Ny, int D, int bins);     /* 0 for sizes slic_pair_stats rejects */
int slic_pair_stats(const float* X, int64_t Nx, int64_t ldx, const int32_t* lx, const float* Y, int64_t Ny, int64_t ldy,
                    const int32_t* ly, int D, int bins, int has_ignore, int32_t ignore_label, double t, uint64_t* hist,
                    double* record, void* workspace, void* stream);

/* ------------------------------------------------------------------------------------------
 * Memory-bank NCE (loss/NCE_loss.py:26-88 NCEAverage, :341-352 NCESoftmaxLoss): gather + dot + /T without
 * materialising the gathered rows, its backward wrt the features, the momentum bank update, and the
 * class-0 softmax cross-entropy.  idx / y are int64 (torch.long) as in the reference.
 * ---------------------------------------------------------------------------------------- */
/* out[b, j] = <bank[idx[b, j], :], f[b, :]> / T      idx: [B, K1], bank: [n_data, D], D % 4 == 0.
 * gathered (optional, [B*K1, D]): the rows as scored, written in the same pass — the training path needs them
 * for the backward because the bank is updated in place right after scoring (NCE_loss.py:73-86). */
int slic_nce_scores_fwd(const float* bank, const int64_t* idx, const float* f, int B, int K1, int D, float T,
                        float* out, float* gathered, void* stream);
/* df[b, :] = (1/T) sum_j dout[b, j] * bank[idx[b, j], :] */
int slic_nce_scores_bwd(const float* bank, const int64_t* idx, const float* dout, int B, int K1, int D, float T,
                        float* df, void* stream);
/* bank[y[b]] = normalise(momentum * bank[y[b]] + (1 - momentum) * f[b])  (NCE_loss.py:73-86) */
int slic_nce_bank_update(float* bank, const int64_t* y, const float* f, int B, int D, float momentum, void* stream);
/* loss = mean_b (logsumexp(x[b, :]) - x[b, 0]); lse/rowloss: [B] scratch kept for the backward */
int slic_softmax_ce0_fwd(const float* x, int B, int K1, float* lse, float* rowloss, float* loss, void* stream);
int slic_softmax_ce0_bwd(const float* x, const float* lse, int B, int K1, const float* gscale, float* dx, void* stream);
/* The contrastive step of online_train.py:175-190 — out_l, out_ab = contrast(feat_l, feat_ab, index); loss =
 * NCESoftmaxLoss(out_l) + NCESoftmaxLoss(out_ab) — as three launches (the separate entry points above: a dozen):
 *   slic_nce_fused_fwd   : scores[0] = <memory_l[idx], f_ab> / T (out_ab), scores[1] = <memory_ab[idx], f_l> / T (out_l), [2][B][K1];
 *                          rows [2][B][K1][D] = the bank rows as scored (the update below changes the banks before the backward);
 *                          part [2][B][SLIC_NCE_PARTS][2] = (max, sum-exp) of each of the SLIC_NCE_PARTS pieces a score row is split into
 *   slic_nce_fused_update: both banks' momentum update (NCE_loss.py:73-86; on duplicate labels the last row wins, every row computed
 *                          from the bank as it was); with part != NULL also lse / rowloss [2][B] = log-sum-exp of a score row and its
 *                          cross-entropy against class 0, and loss = mean_b rowloss[0][b] + mean_b rowloss[1][b]
 *   slic_nce_fused_bwd   : df[0] = d loss / d f_ab, df[1] = d loss / d f_l ([2][B][D]), scaled by *gscale (NULL = 1) */
#define SLIC_NCE_PARTS 16
int slic_nce_fused_fwd(const float* bank_l, const float* bank_ab, const float* f_l, const float* f_ab, const int64_t* idx, int B,
                       int K1, int D, float T, float* scores, float* rows, float* part, void* stream);
int slic_nce_fused_update(float* bank_l, float* bank_ab, const int64_t* y, const float* f_l, const float* f_ab, int B, int D,
                          float momentum, const float* part, const float* scores, int K1, float* lse, float* rowloss, float* loss,
                          void* stream);
int slic_nce_fused_bwd(const float* rows, const float* scores, const float* lse, int B, int K1, int D, float T,
                       const float* gscale, float* df, void* stream);

/* ------------------------------------------------------------------------------------------
 * Classifier head (coclr_classify.py: nn.CrossEntropyLoss() + calc_topk_accuracy(logit, target, (1, 5)) on the `linear` head of
 * models/resnet.py:192-201): mean-reduced softmax cross-entropy with general int64 targets, the rank of the target logit from
 * the same pass, and a dropout whose mask is recomputed from a counter-based generator.
 * ---------------------------------------------------------------------------------------- */
/* logits: [B, C] fp32 with row stride ld >= C (elements); targets: [B] int64.
 *   lse      [B][2]  (row maximum, log of the sum of exp(x - maximum)) — the log-sum-exp in two parts, kept for the backward
 *   rowloss  [B]     log-sum-exp - x[target]
 *   loss     [1]     mean of rowloss (NaN when a target is out of range)
 *   topk_hits int32 [SLIC_CE_HITS_HEAD + B] = {rows whose target is outside [0, C), top-1 hits, top-5 hits, rank[0 .. B)};
 *            rank[b] = #{j : x[b][j] > x[b][t]} + #{j < t : x[b][j] == x[b][t]} (torch.topk's order on distinct values, lower
 *            index first on ties), -1 for a row whose target is out of range — such a row reads no x[b][t] and adds nothing to
 *            the hits; the caller checks topk_hits[0] (an argument error it reports after the launch). */
#define SLIC_CE_HITS_HEAD 3
int slic_softmax_ce_fwd(const float* logits, int64_t ld, int B, int C, const int64_t* targets, float* lse, float* rowloss,
                        float* loss, int32_t* topk_hits, void* stream);
/* dlogits [B, C] dense = (softmax - onehot(target)) * (*gscale, NULL = 1) / B */
int slic_softmax_ce_bwd(const float* logits, int64_t ld, const float* lse, const int64_t* targets, int B, int C,
                        const float* gscale, float* dlogits, void* stream);
/* y[i] = keep(i) ? x[i] / (1 - p) : 0, keep(i) drawn with probability 1 - p from Philox4x32-10 keyed by seed at counter
 * (i / 4, offset): the mask is a function of (seed, offset, i) and is recomputed by the backward, which applies the same map to
 * dy.  p = 1 gives zeros, p = 0 a copy.  This is not torch's dropout stream: the same seed gives a different (equally valid) mask. */
int slic_dropout_fwd(const float* x, int64_t n, float p, uint64_t seed, uint64_t offset, float* y, void* stream);
int slic_dropout_bwd(const float* dy, int64_t n, float p, uint64_t seed, uint64_t offset, float* dx, void* stream);

/* ------------------------------------------------------------------------------------------
 * Segment means for the downstream protocol (coclr_classify.py:575, 622 softmax(logit).mean(0) per view, then the mean over views; :734
 * feature.mean(0)).  x: R rows of C fp32 values, row pitch ld >= C (elements).  The rows fall into V consecutive segments,
 * [seg_off[v], seg_off[v + 1]); for each
 *   table[rows[v]][0 .. C)  (accumulate ? += : =)  w[v] * sum over the segment's rows r, ascending, of f(x_r)
 * with f the identity (mode 0) or the softmax over the C columns (mode 1: expf(x - rowmax) / sum of them).  Every output is ONE
 * sequential fp32 sum in ascending r, compensated (the rounding error of every addition is summed beside it and added at the end,
 * unless it is not finite); w[v] * sum is rounded, then added: no float atomics, the same inputs give the same bits.
 * Rows of table that no segment addresses, and its columns C .. ldt, are not touched.
 * segs: {int32 seg_off[V + 1], int32 rows[V], float w[V]} packed in that order, on the device; segs_host: the same bytes on the
 * host, which the entry point checks before it launches anything: 0 <= seg_off[0], seg_off ascending with no empty segment,
 * seg_off[V] <= R, rows[] distinct and inside [0, table_rows), 1 <= C <= 4096, ld and ldt >= C, mode and accumulate 0 or 1, R, V,
 * table_rows >= 1 — SLIC_EINVAL otherwise (answers without a device).
 * Non-finite inputs propagate as IEEE arithmetic does (a NaN, a +inf, or a row of nothing but -inf gives NaN in that segment's
 * row), except that a -inf logit beside a finite row maximum contributes exactly 0 in mode 1. */
int slic_segment_mean(const float* x, int64_t ld, int R, int C, const void* segs, const void* segs_host, int V, int mode,
                      int accumulate, float* table, int64_t ldt, int table_rows, void* stream);

/* ------------------------------------------------------------------------------------------
 * MoCo queue contrast (loss/NCE_loss.py MemoryMoCo :188-241; the InfoNCE / UberNCE loss of online_train.py:96-97): queries q [B, D]
 * and keys k [B, D] against a dense queue memory [K, D], all row-major fp32, 1 <= D <= 512, K D < 2^29.
 *   logit[b, 0] = <q_b, k_b> / T,  logit[b, 1 + j] = <memory_j, q_b> / T
 * Exact fp32, no float atomics, fixed summation orders: the same inputs give the same bits.  There is no gradient to k or memory.
 * The fused pair slic_moco_ce_fwd / _bwd holds no [B, K] and no [K, D] temporary.
 * ---------------------------------------------------------------------------------------- */
#define SLIC_MOCO_PARTS 256      /* most K-slices of a forward: slic_moco_ce_fwd's workspace is SLIC_MOCO_PARTS * B * 4 floats */
#define SLIC_MOCO_DQ_PARTS 128   /* most K-slices of a backward: its workspace is SLIC_MOCO_DQ_PARTS * B * D floats */
/* out [B, K + 1] = the logits */
int slic_moco_logits_fwd(const float* q, const float* k, const float* memory, int B, int K, int D, float T, float* out,
                         void* stream);
/* dq [B, D] = (dout[:, 0] * k + dout[:, 1:] @ memory) / T; memory: the queue as it was scored */
int slic_moco_logits_bwd(const float* dout, const float* k, const float* memory, int B, int K, int D, float T, float* dq,
                         void* workspace, void* stream);
/* loss = mean_b (lse_b - (sum of row b's positive logits) / npos_b).  Row b's positives: column 0 and, when k_label [B] and
 * queue_label [K] (int64, -1 = empty slot; both or neither) are given, every j with queue_label[j] == k_label[b] >= 0.
 * stat [4][B] = (logit[b, 0], lse_b, npos_b, row loss), kept for the backward.  workspace: 16-byte aligned. */
int slic_moco_ce_fwd(const float* q, const float* k, const float* memory, int B, int K, int D, float T, const int64_t* k_label,
                     const int64_t* queue_label, float* stat, float* loss, void* workspace, void* stream);
/* dq [B, D] = (*gscale, NULL = 1) / (B T) * [ (p_b0 - w_b0) k_b + sum_j (p_bj - w_bj) memory_j ], p = softmax recomputed tile by tile
 * from stat's lse, w = positives / npos; memory, the labels and stat as slic_moco_ce_fwd saw and left them */
int slic_moco_ce_bwd(const float* q, const float* k, const float* memory, int B, int K, int D, float T, const int64_t* k_label,
                     const int64_t* queue_label, const float* stat, const float* gscale, float* dq, void* workspace, void* stream);
/* memory[(index + i) mod K] = k_i for i < B <= K (NCE_loss.py:233-239), queue_label[(index + i) mod K] = k_label[i] when
 * queue_label is given */
int slic_moco_enqueue(float* memory, int64_t* queue_label, const float* k, const int64_t* k_label, int B, int K, int D, int index,
                      void* stream);
/* The top-k accuracy of the same logits without writing them (online_train.py calc_mask_accuracy / calc_topk_accuracy against
 * column 0).  Order the columns of row b by descending logit, ties by ascending column; best(b) = the first positive column in that
 * order (positives as in slic_moco_ce_fwd), rank(b) = the number of columns ahead of it.  rank [B] (NULL = not wanted) =
 * min(rank(b), top_ks[n_ks - 1]); hits[i] = #{b : rank(b) < top_ks[i]}, written, not accumulated.  top_ks is a HOST array of
 * n_ks <= 8 ascending values in 1 .. 8; everything else lives on the device.  Integer results: two runs give the same bits.
 * workspace: 8-byte aligned, SLIC_MOCO_TOPK_WORKSPACE_BYTES(B) bytes.  Limits and SLIC_EINVAL as slic_moco_ce_fwd. */
#define SLIC_MOCO_TOPK_WORKSPACE_BYTES(B) ((size_t)(SLIC_MOCO_PARTS + 1) * (size_t)(B) * 8)
int slic_moco_topk_hits(const float* q, const float* k, const float* memory, int B, int K, int D, float T, const int64_t* k_label,
                        const int64_t* queue_label, const int32_t* top_ks, int n_ks, int32_t* rank, int32_t* hits, void* workspace,
                        void* stream);
/* The same definition on dense logits [B, C] (row pitch ld) and a dense mask [B, C] (uint8, non-zero = positive, row pitch ldm).
 * rank [B] is not saturated; a row without a positive gets rank C and never hits.  top_ks: HOST, n_ks <= 8 ascending values in
 * 1 .. C.  hits [n_ks] is written, not accumulated. */
int slic_mask_topk_hits(const float* logits, int ld, const uint8_t* mask, int ldm, int B, int C, const int32_t* top_ks, int n_ks,
                        int32_t* rank, int32_t* hits, void* stream);
/* torch.nn.functional.normalize(x, dim=1, eps) of dense rows x [B, D] and its backward (models/infoNCE.py:164,177):
 * y = x / max(||x||, eps); inv [B] = 1 / max(||x||, eps), negated for a row the eps clamped, is what the backward keeps.
 * dx = |inv| (dy - y <dy, y>), and dx = dy / eps for a clamped row.  One wave per row, fixed summation order. */
int slic_l2normalize_fwd(const float* x, int B, int D, float eps, float* y, float* inv, void* stream);
int slic_l2normalize_bwd(const float* dy, const float* y, const float* inv, int B, int D, float* dx, void* stream);

/* ------------------------------------------------------------------------------------------
 * Clip transforms (coclr_utils/transforms.py: crop, pad, flip, bilinear resize, brightness / contrast / saturation jitter, random
 * gray, normalise) on a batch of B clips as one gather kernel: uint8 [N, H, W, 3] or fp32 [3, N, H, W] per clip in, fp32
 * [B, 3, N, Ho, Wo] out.  `table` is the device copy and `table_host` the host copy of the per-clip records and factor arrays (layout:
 * the header comment of csrc/cliptf.hip); both entry points check on the host copy that every index a record can produce stays inside
 * its clip and the table.  Built without a*b+c contraction; no atomics; the same inputs give the same bits.
 * ---------------------------------------------------------------------------------------- */
#define SLIC_CLIPTF_REC_BYTES 144
#define SLIC_CLIPTF_MAX_OPS 4
#define SLIC_CLIPTF_BRIGHTNESS 0
#define SLIC_CLIPTF_CONTRAST 1
#define SLIC_CLIPTF_SATURATION 2
#define SLIC_CLIPTF_GRAY 3
#define SLIC_CLIPTF_SRC_U8 0       /* uint8 NHWC, values 0..255 */
#define SLIC_CLIPTF_SRC_U8_255 1   /* uint8 NHWC, divided by 255 */
#define SLIC_CLIPTF_SRC_F32 2      /* fp32 CNHW */
/* bytes of the per-(clip, frame, row band) partial sums a group with a contrast op needs */
size_t slic_clip_transform_workspace_bytes(int B, int N, int Ho, int Wo);
/* workspace <- partial sums of the gray of every frame as it is before its clip's contrast op (clips without one: untouched) */
int slic_clip_transform_stats(const void* table, const void* table_host, size_t table_bytes, int B, int N, int Ho, int Wo, int kind,
                              void* workspace, void* stream);
/* out [B, 3, N, Ho, Wo] (16-byte aligned); normalize: apply the table's mean / std; workspace: what slic_clip_transform_stats left
 * (NULL when no clip has a contrast op) */
int slic_clip_transform_apply(const void* table, const void* table_host, size_t table_bytes, int B, int N, int Ho, int Wo, int kind,
                              int normalize, const void* workspace, float* out, void* stream);

/* ------------------------------------------------------------------------------------------
 * Multi-tensor parameter updates: torch.optim.SGD / torch.optim.Adam (online_train.py:540-543, coclr_classify.py:206-208) and the
 * MoCo key-encoder momentum update (models/infoNCE.py:87-90), each as ONE launch over every tensor of every parameter group.
 *   map        device, int32 [n_items][2]: (tensor, chunk); chunk c is elements [c * CHUNK, (c + 1) * CHUNK) of its tensor,
 *              CHUNK = slic_multi_tensor_chunk().  An entry outside its tensor is skipped, never followed.
 *   desc       device, n_tensors records of SLIC_MT_DESC_BYTES (16-byte aligned):
 *                u64 p, g, s1, s2   parameter, gradient, state (SGD: momentum_buffer, -; Adam: exp_avg, exp_avg_sq; EMA: p = key,
 *                                   g = query, no state); fp32, contiguous, 4-byte aligned
 *                i64 n              elements; offsets are 64-bit throughout, so n > 2^31 does not wrap
 *                i32 flags, pad     SLIC_MT_VEC: every pointer used is 16-byte aligned (float4 path; else element by element)
 *                f64 h[10]          SGD : lr, momentum, 1 - dampening, weight_decay
 *                                   Adam: lr / bc1, 1 - beta1, beta2, 1 - beta2, eps, weight_decay, sqrt(bc2), bc = 1 - beta^step
 *                                   EMA : m, 1 - m
 *                                   LARS: lr, momentum, trust_coefficient (> 0), weight_decay
 *                                   the gradient-only operations (norm modes 1 and 2, scale) read g, n and flags alone: p may be 0
 *                                   computed by the caller in double, rounded to fp32 once on the device
 *   desc_host  the host copy of desc, validated before every launch (pointers, alignment against the flag, state present)
 * Formulas and the rounding of the chains (explicit fmaf, no other contraction): header comment of csrc/optim.hip.
 * Adam is torch's Adam with L2 weight decay (not AdamW, no amsgrad); maximize is not supported.
 * ---------------------------------------------------------------------------------------- */
#define SLIC_MT_DESC_BYTES 128
#define SLIC_MT_HYPER 10
#define SLIC_MT_VEC 1
#define SLIC_MT_NESTEROV 2
#define SLIC_MT_FIRST 4      /* SGD, LARS: this tensor's first step, buf = g' */
#define SLIC_MT_ADAPT 8      /* LARS only: the update is scaled by the tensor's trust ratio; every other operation rejects the flag */
/* chunk length in elements (a multiple of 4) */
int slic_multi_tensor_chunk(void);
/* all_first != 0: every tensor is on its first step (as if each carried SLIC_MT_FIRST), so the table of step 1 serves step 2 */
int slic_multi_sgd(const void* map, int n_items, const void* desc, const void* desc_host, int n_tensors, int all_first, void* stream);
int slic_multi_adam(const void* map, int n_items, const void* desc, const void* desc_host, int n_tensors, void* stream);
int slic_multi_ema(const void* map, int n_items, const void* desc, const void* desc_host, int n_tensors, void* stream);
/* Per-tensor norms over the same two tables, as two launches, and what reads them.  Deterministic: no floating-point atomics, a fixed
 * summation order, so the same inputs give the same bits (order and rounding: header comment of csrc/optim.hip).
 *   slic_multi_sqnorm     partials [n_items][2] doubles (8-byte aligned), one pair per work item, every pair written:
 *                           SLIC_MT_NORM_LARS      {sum p^2, sum u^2}, u = weight_decay != 0 ? fmaf(weight_decay, p, g) : g in fp32 (LARS table)
 *                           SLIC_MT_NORM_GRAD_L2   {0, sum g^2}
 *                           SLIC_MT_NORM_GRAD_INF  {0, max |g|}, NaN if an element is
 *                         elements widened to double, squares and sums in double
 *   slic_multi_norm_fold  the same mode and table; n_items must be the work items the tensors make.  norms [3][n_tensors] fp32 (8-byte
 *                         aligned): wnorm, unorm, q, each rounded once from double; q = (wnorm > 0 && unorm > 0) ?
 *                         trust_coefficient * wnorm / unorm : 1 in SLIC_MT_NORM_LARS, 1 otherwise.  The gradient modes also write total [2] fp32
 *                         (8-byte aligned; may be NULL in SLIC_MT_NORM_LARS): the norm over all tensors, and the coefficient
 *                         min(max_norm * (1 / (total + 1e-6)), 1) in fp32 as torch.nn.utils.clip_grad_norm_ rounds it (NaN stays NaN).
 *                         max_norm must be finite.
 *   slic_multi_lars       the LARS step: u = g + wd p; v = SLIC_MT_ADAPT ? ratios[tensor] u : u; buf = first ? v : mom buf + v; p -= lr buf.
 *                         ratios: the q row of norms (device; may be NULL when no tensor carries SLIC_MT_ADAPT).  A tensor without the
 *                         flag is slic_multi_sgd's chain with dampening 0 and no nesterov, bit for bit.
 *   slic_multi_scale      g *= total[1], read on the device; writes nothing where total[1] >= 1 (NaN is not).  Gradient-only table. */
#define SLIC_MT_NORM_LARS 0
#define SLIC_MT_NORM_GRAD_L2 1
#define SLIC_MT_NORM_GRAD_INF 2
int slic_multi_sqnorm(const void* map, int n_items, const void* desc, const void* desc_host, int n_tensors, int mode, double* partials,
                      void* stream);
int slic_multi_norm_fold(const void* desc, const void* desc_host, int n_tensors, int n_items, const double* partials, int mode,
                         double max_norm, float* norms, float* total, void* stream);
int slic_multi_lars(const void* map, int n_items, const void* desc, const void* desc_host, int n_tensors, int all_first, const float* ratios,
                    void* stream);
int slic_multi_scale(const void* map, int n_items, const void* desc, const void* desc_host, int n_tensors, const float* total, void* stream);

/* Exact t-SNE in two dimensions over a dense N x N fp32 matrix, after sklearn 1.7.2's TSNE(method='exact') (csrc/tsne.hip), and the
 * centred Gram matrix of PCA.  2 <= N <= SLIC_TSNE_MAX_N.  No floating-point atomics: every sum has one fixed order, two runs agree
 * bit for bit.  None of the calls synchronises.
 *   sqdist       d2 [N, N]: d2[i][j] = sum_k (x_ik - x_jk)^2, k ascending, fp32 (X [N, D], row stride ldx >= D, any D >= 1).  Equal
 *                rows give exactly 0; the diagonal is 0.
 *   cond_p       in place over d2: row i becomes p_j|i = exp(-beta_i d_ij) / sum_{k != i} exp(-beta_i d_ik), p_i|i = 0, with beta_i
 *                found by _binary_search_perplexity's rule (at most 100 steps from beta = 1: doubling / halving / bisection until the
 *                entropy is within 1e-5 of log(perplexity)), evaluated on d - min_{k != i} d_ik (the same p, sum >= 1) with the
 *                row sums in double.  beta [N] fp32: the beta of the last step evaluated.
 *   symmetrize   in place: P <- max((P + P^T) / sum(P + P^T), DBL_EPSILON) off the diagonal, 0 on it; P == P^T bit for bit.
 *   step         one iteration of _gradient_descent on Y [N, 2] with its state update [N, 2], gains [N, 2] (all fp32, in place):
 *                w_ij = 1 / (1 + |y_i - y_j|^2), Z = sum_{i != j} w_ij, grad_i = 4 sum_j (e P_ij w_ij - w_ij^2 / Z)(y_i - y_j);
 *                gains += 0.2 where update * grad < 0, else *= 0.8, floor 0.01; update = momentum update - learning_rate gains grad;
 *                Y += update.  grad_out [N, 2] (may be NULL): grad before the gains.  record (SLIC_TSNE_RECORD doubles): Z; the KL
 *                divergence sum_{i != j} e P_ij log(e P_ij Z / w_ij) of the Y the call read (NaN unless want_kl); |gains grad|_2 (the
 *                norm _gradient_descent tests); sum_{i != j} P_ij (NaN unless want_kl).  Three launches.
 *   gram         G [D, D] double = sum_i (x_i - mean)(x_i - mean)^T, products and sums in double, rows ascending inside each of
 *                `shares` equal row ranges, the ranges added in order.  partial: [shares, D, D] doubles of scratch.
 * The workspace of symmetrize and step: slic_tsne_workspace_bytes, 0 for an N outside the limits. */
#define SLIC_TSNE_MAX_N 65536
#define SLIC_TSNE_GRAM_MAX_D 8192
#define SLIC_TSNE_RECORD 4
#define SLIC_TSNE_REC_Z 0
#define SLIC_TSNE_REC_KL 1
#define SLIC_TSNE_REC_GRAD_NORM 2
#define SLIC_TSNE_REC_SUM_P 3
size_t slic_tsne_workspace_bytes(int64_t N);
int slic_tsne_sqdist(const float* X, int64_t N, int D, int64_t ldx, float* d2, void* stream);
int slic_tsne_cond_p(float* P, int64_t N, double perplexity, float* beta, void* stream);
int slic_tsne_symmetrize(float* P, int64_t N, void* workspace, void* stream);
int slic_tsne_step(const float* P, int64_t N, float exaggeration, float momentum, float learning_rate, int want_kl, float* Y,
                   float* update, float* gains, float* grad_out, double* record, void* workspace, void* stream);
int slic_tsne_gram(const float* X, int64_t N, int D, int64_t ldx, const double* mean, int shares, double* partial, double* G,
                   void* stream);

/* ------------------------------------------------------------------------------------------
 * k-NN classification and ranked retrieval metrics on the top-k lists (csrc/knn.hip).
 * ------------------------------------------------------------------------------------------
 * Both calls read [Nq, k] tables as slic_cosine_topk / slic_euclidean_topk / slic_topk_merge_lists write them: int32 gallery rows,
 * distances ascending with ties to the lower row, entries < 0 or >= Ng are padding.  1 <= k <= SLIC_KNN_MAX_K.  Neither takes a
 * workspace, neither synchronises, neither uses a floating-point atomic: the results are a function of the tables alone.
 *
 * slic_knn_vote: the weighted vote of sklearn's KNeighborsClassifier / the k-NN monitor.  g_labels [Ng] int64 are classes 0 .. C - 1,
 * 1 <= C <= SLIC_KNN_MAX_CLASSES.  An entry VOTES unless it is padding or its gallery label is < 0 (noise used as a pseudo-label) or
 * >= C.  With d_j the table's distance of the voting entry at rank j, its weight w_j is
 *   SLIC_KNN_UNIFORM   1                                      (dist may be NULL)
 *   SLIC_KNN_DISTANCE  1 / d_j; if any voting entry of the row has d == 0: (d_j == 0)                     (sklearn's rule)
 *   SLIC_KNN_SOFTMAX   expf((d_first - d_j) * (1 / temperature)), d_first = the distance of the row's first voting entry: every
 *                      weight is <= 1; for cosine distances this is exp(sim_j / T) up to a factor the normalisation removes.
 * s[c] = the float32 sum of the w_j with label c, added one at a time in rank order from 0; tot = the sum of s over the classes: lane l
 * of 64 adds s[l], s[l + 64], ... in that order, then t += t[lane ^ o] for o = 32, 16, .. 1.  Outputs, each may be NULL:
 *   proba [Nq, C]      s[c] / tot
 *   pred  [Nq, n_top]  the n_top classes by (s descending, class ascending) — the lowest class wins a tie, as numpy's argmax does;
 *                      classes nobody voted for take part with s = 0; -1 past the C-th place
 *   score [Nq, n_top]  their s (0 where pred is -1)
 * n_top <= SLIC_KNN_MAX_TOP, 0 exactly when pred and score are both NULL.  A row without a voting entry gets proba = 0, pred = -1,
 * score = 0.  SLIC_EINVAL for sizes outside the limits, an unknown mode, dist == NULL in a mode that weighs, temperature <= 0.
 *
 * slic_retrieval_ranked: with h_j = (g_labels[idx[q, j]] == q_labels[q]) (padding never hits) and c_j = h_0 + .. + h_j, for each of
 * the n_ks <= SLIC_KNN_MAX_CUTS ascending cut-offs K (a HOST array, 1 <= K <= k) and n_rel[q] = how many gallery rows are relevant:
 *   P@K = c_{K-1} / K,  R@K = c_{K-1} / n_rel,  AP@K = (sum_{j < K, h_j} c_j / (j + 1)) / min(n_rel, K),  RR = 1 / (first hit + 1)
 * in double; R and AP are 0 for n_rel <= 0, RR is 0 without a hit in the k entries.  per_query [Nq, n_ks, 3] = (P, R, AP), rr [Nq].
 * record (may be NULL; 3 * n_ks + 2 doubles): the means of the 3 * n_ks columns in per_query's order, the mean of rr, and the number
 * of queries with n_rel > 0.  P and RR average over all Nq queries, R and AP over those with n_rel > 0 (0 when there is none).  A
 * second launch adds each column in double in a fixed order (thread t of 256: queries t, t + 256, ... ascending; then slic_wg_fold's
 * halving). */
#define SLIC_KNN_MAX_K 1024
#define SLIC_KNN_MAX_CLASSES 4096
#define SLIC_KNN_MAX_TOP 8
#define SLIC_KNN_MAX_CUTS 8
#define SLIC_KNN_UNIFORM 0
#define SLIC_KNN_DISTANCE 1
#define SLIC_KNN_SOFTMAX 2
int slic_knn_vote(const int32_t* idx, const float* dist, int Nq, int k, const int64_t* g_labels, int Ng, int C, int mode,
                  float temperature, int n_top, float* proba, int32_t* pred, float* score, void* stream);
int slic_retrieval_ranked(const int32_t* idx, int Nq, int k, const int64_t* q_labels, const int64_t* g_labels, int Ng,
                          const int32_t* n_rel, const int32_t* cutoffs, int n_ks, double* per_query, double* rr, double* record,
                          void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SLIC_HIP_H */
