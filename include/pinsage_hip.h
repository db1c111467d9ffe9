/* pinsage_hip.h -- C ABI of libpinsage_hip.so, the MI355X (gfx950) implementation of the
 * PinSage hot path of anisanazim/Movie-Recommendation-Engine.
 *
 * The reference has no FFI: its boundary for this path is the Python class surface
 * (utils/random_walk.py, model/pinsage.py, model/aggregators.py, utils/nearest_neighbors.py).
 * Each entry point below names the reference code (file:line, relative to the reference
 * root) whose work it replaces; the Python classes of the same names under
 * movie-recommendation-engine_amd/{utils,model}/ bind these symbols with ctypes
 * (see INTEGRATION.md for the stub a maintainer of the reference would add).
 *
 * Conventions
 *  - every pointer is a DEVICE pointer (HBM) unless the parameter name starts with `h_`;
 *    buffers are caller-allocated and caller-owned; inputs are never written.
 *  - `stream` is a hipStream_t passed as void*; all work is enqueued on it, nothing
 *    synchronises, nothing allocates, no state a caller can observe: calls are re-entrant,
 *    callable from several host threads and hipGraph-capturable.  (The only process-wide
 *    data are per-device memos of idempotent one-time queries -- a kernel's dynamic-LDS
 *    attribute has been set, a persistent kernel's resident-workgroup count -- held in
 *    atomics: csrc/ps_common.h PsPerDevice.)
 *  - return value: PS_OK (0) or a negative PS_E* code; `ps_error_string` names it.
 *  - node ids are int32 on the device (V < 2^31), edge offsets int64.
 */
#ifndef PINSAGE_HIP_H
#define PINSAGE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PS_OK 0
#define PS_EINVAL (-1)      /* bad argument / unsupported shape            */
#define PS_ELAUNCH (-2)     /* HIP launch or runtime error                 */
#define PS_EWORKSPACE (-3)  /* workspace too small                         */
#define PS_EUNSUPPORTED (-4)

#define PS_RNG_STREAM 0     /* uniforms[] holds the numpy legacy MT19937 stream */
#define PS_RNG_PHILOX 1     /* Philox4x32-10, counter (node, walk, step/2, call): one block = two steps  */
#define PS_RNG_STREAM_RAW 2 /* ps_walk_sample / ps_walk_sample_layers only: `uniforms` holds the stream as raw MT19937 words
                               (ps_mt19937_raw_stream): uniform i = genrand_res53(temper(word 2i), temper(word 2i+1)) */

#define PS_RNG_STREAM_WALKS 3 /* ps_walk_sample only: PS_RNG_STREAM with ONE stream position per walk, uoff int64[B * W]: step s of
                               walk w of start i reads uniforms[uoff[i * W + w] + s].  For graphs with reachable sinks, where a
                               walk that stops early consumes fewer than L uniforms (utils/random_walk.py:65-69) and the positions
                               are the running count of uniforms consumed by every earlier walk (host: sampling.sink_walk_offsets) */

#define PS_WALK_HALF_BUCKETS 0x100 /* OR-ed into rng_mode of ps_walk_sample / ps_walk_sample_layers: `buckets` holds the 32-byte half
                                      records of ps_bucket_build_half instead of the 64-byte records of ps_bucket_build */

typedef void *ps_stream_t;

int ps_abi_version(void);
const char *ps_error_string(int code);

/* ---- a1: RandomWalkSampler._prepare_adjacency_list (utils/random_walk.py:33-50) -----------
 * adj_list[src].append((dst, w)) in edge-column order  ==  CSR stably sorted by src.
 * src/dst int64[E] (the two rows of edge_index), w float[E] or NULL (=> 1.0, :45-48).
 * Out: rowptr int64[V+1], col int32[E], wsorted double[E] (fp32 weight widened exactly). */
size_t ps_csr_build_workspace_bytes(int64_t E, int64_t V);
int ps_csr_build(const int64_t *src, const int64_t *dst, const float *w, int64_t E, int64_t V,
                 int64_t *rowptr, int32_t *col, double *wsorted,
                 void *workspace, size_t workspace_bytes, ps_stream_t stream);

/* Per-row CDF, the arithmetic `np.random.choice(dest, p=w/w.sum())` performs per step
 * (utils/random_walk.py:76,79): p = w / numpy_sum(w); cdf = cumsum(p); cdf /= cdf[-1], fp64,
 * same operation order (bit-exact).  cdf double[E]. */
int ps_cdf_build(const int64_t *rowptr, const double *wsorted, int64_t V, double *cdf, ps_stream_t stream);

/* Acceleration records for the walk kernels (exact, results unchanged):
 *  nodeinfo uint32[2V] : (row start, out-degree) of every node in one 8-byte record;
 *  guide    int32[E]   : guide[lo_v + j] = #{k : cdf_v[k] <= (j/deg_v)(1 - 2^-50)}, j = 0..deg_v-1 -- a bucket table
 *  for the inverse-CDF lookup: searchsorted(cdf_v, u, 'right') starts at guide[lo_v + floor(u*deg_v)] and
 *  scans forward (usually 1-2 entries) instead of probing log2(deg) cache lines; the threshold sits a hair
 *  below j/deg so that fp64 rounding of u*deg can never put the start past the answer. */
int ps_guide_build(const int64_t *rowptr, const double *cdf, int64_t V, uint32_t *nodeinfo, int32_t *guide,
                   ps_stream_t stream);

/* Packed edge blocks: every 8 consecutive edges e = 8b..8b+7 become one 128-byte line
 *   [ 8 x fp64 cdf | 8 x int32 col | 8 x int32 guide ]   (packed: 128 * ceil(E/8) bytes, 128-B aligned)
 * so the bucket lookup, the CDF scan and the destination read of one walk step usually hit the same line. */
int ps_pack_edges(const int32_t *col, const double *cdf, const int32_t *guide, int64_t E, void *packed,
                  ps_stream_t stream);

/* Bucket records: one 64-byte record per bucket e = lo_v + j of the guide table,
 *   [ c0 c1 | c2 c3 | k0 k1 k2 k3 | c4 k4 - ]   ci fp64 = cdf[lo_v + guide[e] + i], ki int32 = col[same]
 * (past the row end: ci = 2.0, ki = the row's last destination), so searchsorted(cdf_v, u, 'right') = first i with
 * ci > u is answered from ONE 64-byte sector per walk step; a lane that needs more than five candidates repeats the
 * search through the packed blocks.  buckets: 64 * E bytes, 64-B aligned.  Optional (4x the adjacency's memory). */
int ps_bucket_build(const int64_t *rowptr, const int32_t *col, const double *cdf, const int32_t *guide, int64_t V,
                    int64_t E, void *buckets, ps_stream_t stream);

/* The same table at half the size for graphs whose 64-byte records do not fit (BASELINE config 5: 2 x 10^9 edges = 64 GB instead of
 * 128): record lo[v] + j = [lo32(cdf[g]) .. lo32(cdf[g+3]) | col[g] .. col[g+3]] with g the bucket's guide position and lo32 = the
 * fp64 value rounded DOWN to fp32 (cdf lies in [lo32, next float): u < lo32 proves u < cdf, u >= the next float proves u >= cdf);
 * positions past the row end as in ps_bucket_build (2.0f / the row's last destination).  A step is answered from its 32-byte
 * record when these bounds prove one of the four candidates to be the searchsorted pick; a u inside a rounding sliver, or beyond
 * the fourth candidate, makes the walk kernel repeat the search through the packed blocks.  Same results bit for bit.
 * buckets: 32 * E bytes, 64-B aligned; pass PS_WALK_HALF_BUCKETS with the RNG mode. */
int ps_bucket_build_half(const int64_t *rowptr, const int32_t *col, const double *cdf, const int32_t *guide, int64_t V,
                         int64_t E, void *buckets, ps_stream_t stream);

/* Destination records: dest_info[e] = the nodeinfo record (row start, degree) of col[e], 8 bytes per edge, 8-B aligned.  Read
 * contiguously with a start row (the walk kernels stage it into LDS next to the row's blocks), it tells a walk the row of the
 * node it has just picked without a gather of its own: step 1 of a walk is then ONE dependent round trip to memory (the bucket
 * record) instead of two.  Pays where the node records themselves are not cache resident (V * 8 bytes beyond the L2 / MALL:
 * BASELINE config 5, 110 M nodes); optional. */
int ps_dest_info_build(const int32_t *col, const uint32_t *nodeinfo, int64_t E, int64_t V, void *dest_info, ps_stream_t stream);

/* flags[0] = 1 iff some edge points at a node with out-degree 0 (a reachable sink: the
 * reference's walk then breaks early, utils/random_walk.py:68-69, and its RNG consumption
 * becomes data dependent); flags[1] = max out-degree.  flags int64[2]. */
int ps_graph_stats(const int64_t *rowptr, const int32_t *col, int64_t E, int64_t V, int64_t *flags,
                   ps_stream_t stream);

/* ---- a2-a4: _single_walk / sample_neighbors / batch_sample_neighbors (utils/random_walk.py:52-142)
 * For each start node: W walks of L weighted steps (pick = searchsorted(cdf, u, 'right')),
 * visit counts over walk[1:], top-T by (count desc, first-visit order), one wave per start node.
 * rng_mode PS_RNG_STREAM: step (walk w, step s) of start i reads uniforms[uoff[i] + w*L + s]
 *   (uoff int64[B]; the numpy call order on a graph without reachable sinks).
 * rng_mode PS_RNG_STREAM_WALKS: uoff int64[B * W], one position per walk (graphs with reachable sinks; see the define).
 * rng_mode PS_RNG_PHILOX: uniforms/uoff ignored; u = philox(seed; node, w, s/2, call) words (0,1) for even s, (2,3) for odd s.
 * Out: ids int32[B,T] (-1 pad), counts int32[B,T] (0 pad), nvalid int32[B].
 * The reference's weights are counts[i,j] / sum_j counts[i,:nvalid[i]] (:113-115).
 * nodeinfo/guide (both or neither; from ps_guide_build) select the bucket-table lookup; NULL = plain
 * binary search over the CDF row.  packed (from ps_pack_edges; needs nodeinfo) reads cdf/col/guide from
 * the interleaved 128-byte blocks instead of the three arrays; start rows of up to ~40 blocks are searched in LDS.
 * With packed, col / cdf / guide may be NULL (the blocks hold the same values: graphs that fill the GPU drop the plain arrays).
 * buckets (from ps_bucket_build; needs nodeinfo) answers every other step from one 64-byte record; with PS_WALK_HALF_BUCKETS
 * OR-ed into rng_mode it is the 32-byte form of ps_bucket_build_half.
 * dest_info (from ps_dest_info_build; needs packed; may be NULL): the (row start, degree) record of every edge's destination. */
int ps_walk_sample(const int64_t *rowptr, const int32_t *col, const double *cdf, int64_t V,
                   const int64_t *starts, int64_t B, int W, int L, int T,
                   int rng_mode, const double *uniforms, const int64_t *uoff,
                   uint64_t seed, uint32_t call, const uint32_t *nodeinfo, const int32_t *guide,
                   const void *packed, const void *buckets, const void *dest_info,
                   int32_t *ids, int32_t *counts, int32_t *nvalid, ps_stream_t stream);

/* PinSage.get_embeddings draws one fresh sample per GCN layer for the SAME start nodes (model/pinsage.py:271-275:
 * `for layer in range(num_layers): batch_sample_neighbors(nodes, num_neighbors)`).  This entry point runs `layers`
 * consecutive samples of every start node in one wave: the start row is brought into LDS once and the per-node fixed
 * chain (start id -> row bounds -> row) is paid once (few start nodes -- a rank's shard -- get one wave per (node, layer)
 * instead: shorter waves fill the last generation of resident waves better).  Results are exactly those of `layers` ps_walk_sample calls:
 * PS_RNG_PHILOX uses call, call + 1, ...; PS_RNG_STREAM reads layer r's uniforms at r * layer_stride + uoff[i] + w*L + s
 * (layer_stride = the uniforms one whole batch consumes = total[0] of ps_uniform_offsets, i.e. the reference's order:
 * all of layer 0's draws, then all of layer 1's).  ids/counts int32[layers, B, T], nvalid int32[layers, B]. */
int ps_walk_sample_layers(const int64_t *rowptr, const int32_t *col, const double *cdf, int64_t V,
                          const int64_t *starts, int64_t B, int W, int L, int T,
                          int rng_mode, const double *uniforms, const int64_t *uoff, int64_t layer_stride,
                          uint64_t seed, uint32_t call, const uint32_t *nodeinfo, const int32_t *guide,
                          const void *packed, const void *buckets, const void *dest_info, int layers,
                          int32_t *ids, int32_t *counts, int32_t *nvalid, ps_stream_t stream);

/* _single_walk (utils/random_walk.py:52-83), batched: one walk of L steps per start node, one lane
 * per walk.  paths int32[B,L]: the visited nodes after the start (-1 once the walk hit a sink).
 * PS_RNG_STREAM: walk i, step s reads uniforms[uoff[i] + s]; PS_RNG_PHILOX: philox(seed; node, w, s/2, call)
 * with walk id w = i (walk_mod == 0) or i % walk_mod (replays walk w of ps_walk_sample when the start
 * nodes are repeated W = walk_mod times). */
int ps_walk_paths(const int64_t *rowptr, const int32_t *col, const double *cdf, int64_t V,
                  const int64_t *starts, int64_t B, int L, int rng_mode, const double *uniforms,
                  const int64_t *uoff, uint64_t seed, uint32_t call, int walk_mod,
                  const uint32_t *nodeinfo, const int32_t *guide, int32_t *paths, ps_stream_t stream);

/* Node2vec-biased walks: RandomWalkSampler's p (return) and q (in-out), csrc/walk_biased.hip.  ps_walk_paths with one change: on
 * every step that has a previous node t (the second step of a walk onwards) the weights of the row v the walk stands on are
 * multiplied elementwise by alpha before `probabilities = weights / weights.sum()` (utils/random_walk.py:76), alpha of the edge
 * v -> x being  bias[0] = 1/p if x == t,  else 1.0 if t has an out-edge to x,  else bias[1] = 1/q  (parallel edges are judged by
 * their destination).  The rest is numpy's, as in ps_cdf_build: w * alpha one fp64 rounding, numpy's pairwise sum, the
 * sequential cumsum, cdf /= cdf[-1], pick = searchsorted(cdf, u, 'right'); one uniform per step taken, none at a sink.  The first
 * step has no previous node and is searched in `cdf`.  bias = {1, 1} gives ps_walk_paths' paths bit for bit.
 * wsorted double[E] (ps_csr_build), nbr_sorted int32[E]: every row's destinations in ascending order, duplicates kept (the set
 * test is a binary search in t's row).  bias: a DEVICE array of two doubles -- it is not read on the host, so an entry that is
 * not finite and positive is answered on the device: every path of the call is -1 throughout.  PS_RNG_STREAM: walk i, step s
 * reads uniforms[uoff[i] + s] (uoff int64[B], one stream position per walk); PS_RNG_PHILOX and walk_mod as in ps_walk_paths.
 * A start, a previous node or a row offset outside the graph is an isolated node: nothing is read for it.
 * One wave per walk; a step costs O(deg(v) log deg(t)) and O(deg(v)) of it is a sequential fp64 chain (the cumsum).  No
 * workspace.  paths int32[B,L] (-1 after a sink).  PS_OK for B == 0; PS_EINVAL for L < 1 or (B > 0) a null pointer.
 *
 * ps_paths_topk: the visit counting and top-T cut of ps_walk_sample over GIVEN paths: paths int32[B, n] (the n = W * L entries of
 * a start node, walk 0's steps first; negative entries are skipped) -> ids int32[B,T] (-1 pad), counts int32[B,T] (0 pad),
 * nvalid int32[B], ordered by count descending, ties by first visit.  One wave per start node, the entries in LDS.
 * n above ps_paths_topk_max_entries() (4096): PS_EUNSUPPORTED; PS_OK for B == 0; PS_EINVAL for n < 1, T < 1 or (B > 0) a null
 * pointer. */
int ps_walk_paths_biased(const int64_t *rowptr, const int32_t *col, const double *wsorted, const double *cdf,
                         const int32_t *nbr_sorted, int64_t V, const int64_t *starts, int64_t B, int L, int rng_mode,
                         const double *uniforms, const int64_t *uoff, uint64_t seed, uint32_t call, int walk_mod,
                         const double *bias, int32_t *paths, ps_stream_t stream);
int ps_paths_topk_max_entries(void);
int ps_paths_topk(const int32_t *paths, int64_t B, int n, int T, int32_t *ids, int32_t *counts, int32_t *nvalid,
                  ps_stream_t stream);

/* Offsets into the numpy stream: uoff[i] = W*L * #{j < i : outdeg(starts[j]) > 0};
 * total[0] = uniforms consumed by the whole batch. */
int ps_uniform_offsets(const int64_t *rowptr, int64_t V, const int64_t *starts, int64_t B, int W, int L,
                       int64_t *uoff, int64_t *total, ps_stream_t stream);

/* numpy legacy MT19937 `random_sample` on the device: state uint32[624] + pos (0..624) in; `skip` doubles are
 * skipped, then n doubles written; the state after skip + n draws comes back (what np.random.set_state needs).
 * Replaces the global-RNG draws of np.random.choice at utils/random_walk.py:79.
 * jump_polys uint32[jump_levels, 624] (row m = t^(2^m) mod phi over GF(2), from pinsage_hip/mtjump.py) enables
 * the parallel path (2^c-word chunks, c = ps_mt19937_chunk_log2(), generated by independent workgroups, windows by
 * jump-ahead); with NULL polynomials / workspace a single workgroup generates the stream serially (skip must be 0).
 * radix_polys uint32[radix_levels, 31, 624] (entry (i, j-1) = t^(j * 2^(c + 5i)) mod phi, optional): the chunk windows
 * are then produced in radix-32 rounds instead of by doubling.
 * window_polys uint32[n_window, 624] (row j-1 = t^(j * 2^c + s) mod phi, s = ps_mt19937_window_shift() -- the generator
 * expands the sequence s words back from the first window as well as forwards; optional; mtjump.window_polynomials):
 * requests of 33 .. n_window + 1 chunks get ALL their windows in one product round from the first window.
 * ranges (ps_mt19937_raw_stream only; a HOST array int64[n_ranges][2], n_ranges <= 3, NULL = everything): runs [lo, hi) of
 * uniform indices the caller will read -- a rank of an item-sharded job passes the stream positions of ITS start nodes
 * (one run per GCN layer); only those words of `raw` (and the state hand-back) are generated, the rest of the buffer is
 * left unwritten.  The returned state is the post-whole-stream state either way.  Needs window_polys (else ignored). */
/* ps_mt19937_raw_stream: the same stream (skip = 0) left as untempered 32-bit state words in raw uint32[2n + 1248] for
 * PS_RNG_STREAM_RAW -- the walk kernel tempers and combines the two words of a uniform itself, which saves the conversion
 * pass (65 us and 190 MB of traffic per 23.6 M doubles).  Needs the jump polynomials (n >= 2^17). */
int ps_mt19937_chunk_log2(void);
int ps_mt19937_window_shift(void);
int ps_mt19937_raw_stream(const uint32_t *state_in, int pos_in, int64_t n, uint32_t *raw, uint32_t *state_out,
                          int32_t *pos_out, const uint32_t *jump_polys, int jump_levels, const uint32_t *radix_polys,
                          int radix_levels, const uint32_t *window_polys, int n_window, const int64_t *ranges,
                          int n_ranges, void *workspace, size_t workspace_bytes, ps_stream_t stream);
size_t ps_mt19937_workspace_bytes(int64_t skip, int64_t n);
int ps_mt19937_random_sample(const uint32_t *state_in, int pos_in, int64_t skip, int64_t n, double *out,
                             uint32_t *state_out, int32_t *pos_out, const uint32_t *jump_polys, int jump_levels,
                             const uint32_t *radix_polys, int radix_levels, const uint32_t *window_polys, int n_window,
                             void *workspace, size_t workspace_bytes, ps_stream_t stream);

/* ---- a5 / a9: ImportancePooling.forward (model/pinsage.py:101-150); Weighted/Mean/Importance
 * aggregators' gather + weighted reduce (model/aggregators.py:13-91,233-287).
 * x float[N,H]; ids/counts int32[B,T]; nvalid int32[B]; out float[B,H].
 * Row i: keep j < nvalid[i] with 0 <= ids[i,j] <= max_idx (:123-129); w_j = fp32(count_j/total);
 * w /= sum(w) if > 0 (:140-143); out = sum_j w_j * x[ids_j] (:146); zeros if none (:115-117,:132-134).
 * If wts != NULL (float[B,T]) it supplies w_j directly instead of counts (list API with arbitrary
 * weights; aggregators).  renorm = 0 skips the `w /= sum(w)` step (weights already final).
 * nvalid[i] above T means T (nothing is read beyond row i's T entries) and a negative nvalid[i] means 0, here and in
 * ps_gcn_layer.  max_idx above N - 1 means N - 1.  `total` is the int32 sum of counts[i, j < nvalid[i]], dropped ids included.
 * Arithmetic (oracle/pinsage_oracle.c: orc_importance_pool_ex restates it bit for bit): dropped entries carry weight +0; the
 * fp32 sum of the weights is a pairwise tree over the lanes that hold them (entry e in lane e % 16 of a 16-lane group for
 * T <= 64 with H % 4 == 0 and 16-byte aligned x / out; in lane e % 64 of the wave otherwise), the division by it an IEEE fp32
 * division, and out[i, c] the chain acc = fmaf(x[ids_j, c], w_j, acc) over j = 0 .. nvalid[i] - 1 from +0.  For T <= 16 both
 * lane layouts give the same bits. */
int ps_importance_pool(const float *x, int64_t N, int H, const int32_t *ids, const int32_t *counts,
                       const float *wts, const int32_t *nvalid, int64_t B, int T, int64_t max_idx,
                       int renorm, float *out, ps_stream_t stream);

/* ---- a9: AttentionAggregator's scores + softmax (model/aggregators.py:131-151) and MaxPoolingAggregator's maximum over the
 * neighbours' transformed rows (:195-209), csrc/neigh_agg.hip.  Both keep slot j of row i iff j < min(nvalid[i], T) and
 * 0 <= ids[i,j] < N (a negative nvalid[i] means 0); no other id is dereferenced.  Caller-allocated buffers, no allocation, no
 * synchronisation; PS_EINVAL for a non-positive Hd / H / T or (B > 0) a null pointer; PS_OK for B == 0, whatever the
 * pointers (the base of an empty buffer may be NULL).
 *
 * ps_attention_weights: u float[B,Hd], v float[N,Hd], w2 float[Hd], ids int32[B,T], nvalid int32[B], attn float[B,T].
 * The attention MLP Linear(2C -> C), ReLU, Linear(C -> 1) over cat([self, neighbour]) (:147-150) with the first layer split by
 * columns: u = self_features W1[:, :C]^T + b1 and v = features W1[:, C:]^T are two ps_linear calls, w2 the second layer's
 * weight.  s_ij = sum_c w2[c] * max(u[i,c] + v[ids[i,j],c], 0) for a kept slot; attn[i,:] = softmax of the kept scores (row
 * maximum subtracted, exponentials divided by their sum, :151); +0.0 in every slot that is not kept, all zeros for a row that keeps
 * nothing (:132-135).  The second layer's bias shifts every score of a row alike and drops out of the softmax: it is not an
 * argument.  The weighted sum of :154-157 is ps_importance_pool(x, ..., wts = attn, renorm = 0).
 *
 * ps_gather_max: x float[N,H], out float[B,H].  out[i,c] = max over the kept slots of x[ids[i,j], c], from -inf (never from 0);
 * a NaN among the gathered values gives NaN (torch.max, :208); +0.0 in every column of a row that keeps nothing (:196-199).
 * x is the MLP's output over all rows (ps_linear with PS_RELU), computed once instead of once per neighbour list. */
int ps_attention_weights(const float *u, const float *v, int64_t N, int Hd, const float *w2, const int32_t *ids,
                         const int32_t *nvalid, int64_t B, int T, float *attn, ps_stream_t stream);
int ps_gather_max(const float *x, int64_t N, int H, const int32_t *ids, const int32_t *nvalid, int64_t B, int T, float *out,
                  ps_stream_t stream);

/* ---- a9, backward: the gradients of the three neighbour gathers above (ps_importance_pool, ps_attention_weights followed by
 * ps_importance_pool, ps_gather_max), csrc/neigh_agg_bwd.hip.  The backward of a gather is a scatter; it is computed as a gather
 * over the TRANSPOSED index, so no float is added atomically and every output bit is a function of the inputs.  Caller-allocated
 * buffers, no allocation, no synchronisation; PS_OK for an empty problem (B == 0, or N == 0 where N is the row count of the
 * output), whatever the pointers; PS_EINVAL for a non-positive width / T, a null pointer on a non-empty problem or a short
 * workspace.  Workspaces are not preserved between calls and need no alignment.
 *
 * Slot lists.  A slot is s = i * T + j (B * T < 2^31, else PS_EINVAL).  rptr int64[N + 1] / slots int32[nnz] list, per feature row
 * r, the KEPT slots whose id is r: S(r) = slots[rptr[r] .. rptr[r + 1]), ascending; rptr[0] = 0, rptr non-decreasing,
 * rptr[N] = nnz <= B * T (pinsage_hip/sampling.py: slot_lists).  Offsets are clamped to [0, B * T] on the device and a slot outside
 * [0, B * T) contributes nothing, so no access leaves g / coef / arg; the caller guarantees that slots holds rptr[N] entries.
 * Segments: S(r) is cut into consecutive segments of SEG = ps_gather_bwd_segment() slots (a compile-time constant); every segment
 * is its own chain from +0.0 and a row's result is ((p_0 + p_1) + p_2) + ... over its segment results in ascending order (p_0
 * alone for a row of at most SEG slots).  An empty S(r) gives +0.0 in every column; every element of the output is written.
 *
 * ps_pool_weights: w_eff float[B,T] = the weight ps_importance_pool multiplies x[ids[i,j]] by, bit for bit -- the keep rule,
 *   fp32(count / total), the lane-tree sum and the IEEE division of the a5 / a9 block above -- and +0.0 in every slot that is not
 *   kept.  lanes selects the tree: 16 = entry e in lane e % 16 of a 16-lane group, what ps_importance_pool uses for T <= 64 with
 *   H % 4 == 0 and 16-byte aligned x / out (csrc/pool_row.h: pool4_weights, the forward's own code); 64 = lane e % 64 of the wave.
 *   lanes = 16 with T > 64 means 64, as in the forward; any other value: PS_EINVAL.  max_idx is taken as given (the forward clamps
 *   it to N - 1: pass the clamped value).  ps_importance_pool(x, wts = w_eff, renorm = 0) repeats the forward's bits.
 *
 * ps_gather_bwd: g float[B,H], gx float[N,H]; exactly one of coef float[B*T] and arg int32[B,H] is given (else PS_EINVAL).
 *   coef: gx[r,c] = the chain acc = fmaf(coef[s], g[s / T, c], acc) over the slots s of a segment, ascending, from +0.0 -- the
 *         gradient of ps_importance_pool with coef = w_eff, of the attention sum with coef = attn;
 *   arg : acc = acc + g[i,c] over those slots s = i * T + j of the segment with arg[i,c] == j -- the gradient of ps_gather_max_arg.
 *   workspace: ps_gather_bwd_workspace_bytes(B, T, H).  B == 0 with N > 0 writes zeros.  Two launches: the segment chains
 *   (a row of at most SEG slots goes straight to gx), then the sums of the cut rows.
 *
 * ps_gather_max_arg: ps_gather_max (same out, bit for bit) with arg int32[B,H]: the lowest kept slot j holding a NaN in column c
 *   if there is one, otherwise the lowest kept slot whose value equals the maximum; -1 for a row that keeps nothing.
 *
 * ps_attention_bwd_rows: the gradient of out[i] = sum_j attn[i,j] x[ids[i,j]], attn = ps_attention_weights(u, v, w2), with respect
 *   to the scores and to everything that is indexed by the target row.  x float[N,H], g float[B,H] (the gradient of out), attn as
 *   the forward wrote it; one wave per target row, the keep rule of ps_attention_weights.
 *     da_ij = sum_c g[i,c] x[id,c]: lane l chains part = fmaf(g[i,c], x[id,c], part) over its columns (c = 64 V k + V l + e, sweep k
 *             and element e ascending; V = 4 when H % 4 == 0, Hd % 4 == 0 and x, u, v, w2, g, du are 16-byte aligned, else 1) from
 *             +0.0, columns past H entering as 0 * 0, then the 64 lanes are added by the balanced tree of ps_attention_weights;
 *     dot_i = the chain fmaf(attn[i,j], da_ij, acc) over the kept j, ascending, from +0.0;
 *     ds[i,j] = attn[i,j] * (da_ij - dot_i), the difference rounded first; +0.0 in every slot that is not kept (ds float[B,T]);
 *     du[i,c] = the chain fmaf(ds[i,j], (u[i,c] + v[id,c] > 0 ? w2[c] : 0), acc) over the kept j (du float[B,Hd]);
 *     share_i[c] = the chain fmaf(ds[i,j], relu(u[i,c] + v[id,c]), acc) with the forward's relu (h < 0 ? +0 : h);
 *     dw2[c] (float[Hd]) = the sum of the shares in an order that depends on B only: the rows are cut into ceil(B / 128)
 *             partitions of 128 consecutive rows, a partition is acc = acc + share_i[c] over its rows ascending from +0.0, and
 *             dw2[c] is acc = acc + partition_p[c] over the partitions ascending from +0.0.
 *   workspace: ps_attention_bwd_rows_workspace_bytes(B, Hd).  T > 64 works: da is parked in ds between the passes.
 *   Three launches.  dx of the sum is ps_gather_bwd(coef = attn); the second attention layer's bias drops out of the softmax, so
 *   its gradient is exactly zero.
 *
 * ps_attention_bwd_cols: dv float[N,Hd]: dv[r,c] = the chain fmaf(ds[s], (u[s / T, c] + v[r,c] > 0 ? w2[c] : 0), acc) over S(r), with
 *   the segment rule and the two launches of ps_gather_bwd; workspace: ps_gather_bwd_workspace_bytes(B, T, Hd). */
int ps_pool_weights(const int32_t *ids, const int32_t *counts, const float *wts, const int32_t *nvalid, int64_t B, int T,
                    int64_t max_idx, int renorm, int lanes, float *w_eff, ps_stream_t stream);
int ps_gather_bwd_segment(void);
size_t ps_gather_bwd_workspace_bytes(int64_t B, int T, int H);
int ps_gather_bwd(const int64_t *rptr, const int32_t *slots, int64_t N, int T, const float *coef, const int32_t *arg,
                  const float *g, int64_t B, int H, float *gx, void *workspace, size_t workspace_bytes, ps_stream_t stream);
int ps_gather_max_arg(const float *x, int64_t N, int H, const int32_t *ids, const int32_t *nvalid, int64_t B, int T, float *out,
                      int32_t *arg, ps_stream_t stream);
size_t ps_attention_bwd_rows_workspace_bytes(int64_t B, int Hd);
int ps_attention_bwd_rows(const float *x, int64_t N, int H, const float *u, const float *v, int Hd, const float *w2,
                          const int32_t *ids, const int32_t *nvalid, const float *attn, const float *g, int64_t B, int T, float *ds,
                          float *du, float *dw2, void *workspace, size_t workspace_bytes, ps_stream_t stream);
int ps_attention_bwd_cols(const int64_t *rptr, const int32_t *slots, int64_t N, int T, const float *ds, const float *u,
                          const float *v, int Hd, const float *w2, int64_t B, float *dv, void *workspace, size_t workspace_bytes,
                          ps_stream_t stream);

/* ---- a9 (model/layers.py): nn.BatchNorm1d of GraphConvLayer.forward with the ReLU and F.normalize behind it (model/layers.py:68-75),
 * csrc/batch_norm.hip.  Caller-allocated buffers, no allocation, no synchronisation, no atomics.
 *
 * ps_bn_batch_stats: z float[M,N] (dense rows), gamma float[N] -> mean, var, scale float[N], always written:
 *   S = sum_r z[r,c], Q = sum_r z[r,c]^2, both accumulated in fp64 (the square of an fp32 value is exact there) in ONE pass over z;
 *   mean = fp32(S / M); var64 = max(Q / M - (S / M)^2, 0), the biased batch variance, var = fp32(var64);
 *   scale = fp32(gamma / sqrt(var64 + eps)), in fp64.
 * running_mean / running_var float[N], both or neither (one alone: PS_EINVAL), are updated in place, in fp64 with one rounding:
 *   running_mean = (1 - momentum) running_mean + momentum S / M,
 *   running_var  = (1 - momentum) running_var  + momentum var64 M / (M - 1)     (the unbiased variance, as torch tracks it).
 * eps and momentum arrive as fp32 -- the precision torch's own fp32 kernels use them at -- and are widened to fp64.
 * Summation order: the rows are cut into ceil(M / 128) partitions of 128 consecutive rows (a function of M only); within a
 * partition four strided row subsets are summed sequentially and added in subset order; the partitions are added in ascending
 * order.  Equal inputs give equal bits, whatever the workspace held before the call.
 * workspace: ps_bn_stats_workspace_bytes(M, N) bytes (16 N bytes per partition), 8-byte aligned, not preserved between calls.
 * PS_EINVAL for M < 2 (the unbiased variance does not exist), N < 1, a null pointer or a short workspace.
 *
 * ps_bn_apply: y[r,c] = epilogue(fmaf(z[r,c] - mean[c], scale[c], beta[c])), one wave per row.  flags: PS_RELU (t < 0 ? +0 : t),
 * PS_L2NORM (the row divided by nrm = sqrtf(sum_c t^2), 1e-12f where nrm < 1e-12f -- a NaN norm stays, so a row with a NaN is NaN
 * throughout, as F.normalize's clamp_min leaves it; the sum is a per-lane fmaf chain over the lane's columns in
 * ascending order, then the wave sum of the other row kernels); any other bit: PS_EINVAL.  y may be z: in place gives the bits of
 * out of place.  PS_OK for M == 0, whatever the pointers; PS_EINVAL for N < 1 or (M > 0) a null pointer.
 * With mean = running_mean and scale = gamma / sqrt(running_var + eps) this is eval-mode batch norm. */
size_t ps_bn_stats_workspace_bytes(int64_t M, int N);
int ps_bn_batch_stats(const float *z, int64_t M, int N, const float *gamma, float eps, float momentum, float *running_mean,
                      float *running_var, float *mean, float *var, float *scale, void *workspace, size_t workspace_bytes,
                      ps_stream_t stream);
int ps_bn_apply(const float *z, int64_t M, int N, const float *mean, const float *scale, const float *beta, int flags, float *y,
                ps_stream_t stream);

/* ---- a6: the dense layers of PinSage.forward (model/pinsage.py:202,235-240,248-249) ---------
 * y[M,N] = epilogue( x[M,K] W[N,K]^T (+ x2[M,K2] W2[N,K2]^T) + b ), fp32 MFMA, k-ordered fma chain.
 * x2/W2 eliminate torch.cat([h_self, h_neigh]) (:238): W = lin_update.weight[:, :H], W2 = [:, H:]
 * (ldw / ldw2 = row strides of W / W2 in floats).  flags: PS_RELU, PS_L2NORM (F.normalize, eps 1e-12), PS_WPERM: W (and W2)
 * are stored in the order the kernel stages them (ps_permute_k; needs 16-byte aligned operands and K % 32 == 0, else PS_EINVAL):
 * same results bit for bit, 32 fewer vector instructions per 64 MFMAs -- for weights that are multiplied many times.
 * Per output, fp32: acc = fmaf(x[m,k], W[n,k], acc) over k ascending from +0.0, then the same over x2 / W2; each of the two chains
 * runs on to a multiple of 32 k over terms +0.0 * +0.0 (which turn an accumulator of -0.0 into +0.0 and change nothing else);
 * t = acc + b[n], or acc + 0.0f when b is NULL.  NaN and infinities follow IEEE 754 through the chain: a NaN or Inf - Inf
 * anywhere in it is a NaN output.
 * PS_RELU: t > 0 or t is NaN ? t : +0.0 (so -0.0 gives +0.0, unlike ps_bn_apply).
 * PS_L2NORM: the row divided by nrm = sqrtf(sum_n t^2), 1e-12f where nrm < 1e-12f -- a NaN norm stays, so a row with a NaN is NaN
 * throughout, as F.normalize's clamp_min leaves it; an infinite norm gives Inf / Inf = NaN and +-0.0 for the finite columns.  The
 * quotient is the correctly rounded t / nrm. */
#define PS_RELU 1
#define PS_L2NORM 2
#define PS_WPERM 4
/* out float[rows, K] (dense) = W with every group of eight k as k 0 2 4 6 1 3 5 7 (K % 8 == 0; ld = row stride of W). */
int ps_permute_k(const float *W, int64_t rows, int K, int ld, float *out, ps_stream_t stream);
int ps_linear(const float *x, int64_t M, int K, const float *W, int ldw, const float *b, int N,
              const float *x2, int K2, const float *W2, int ldw2, int flags, float *y, ps_stream_t stream);

/* ---- the same layers under loss.backward() (model/pinsage.py:202,235-240,248-249 on the tape; train.py:72-82), csrc/linear_bwd.hip:
 * the weight and bias gradients of y = epilogue(x W^T + b) and the backward of the epilogue.  (The input gradient g W is ps_linear
 * over W^T, a chain over n ascending.)  Caller-allocated buffers, no allocation, no synchronisation, no float atomics: every output
 * bit is a function of the inputs, whatever the workspace held before the call.
 *
 * ps_linear_wgrad: g float[M,N] (the gradient of the pre-activation), x float[M,K], both dense -> dW float[N,K] (dense) and, unless
 *   db is NULL, db float[N].
 *   Partitions.  The rows are cut into partitions of P = ps_linear_wgrad_partition(M) consecutive rows: P = 512, doubled while
 *   ceil(M / P) > 256 -- a function of M alone (not of N, K, the device, the environment or the alignment of the operands).
 *   s_p[n,k] is the chain acc = fmaf(g[m,n], x[m,k], acc) over the rows m of partition p ascending, from +0.0.
 *   dW[n,k] = ((s_0 + s_1) + s_2) + ... in partition order; s_0 alone when M <= P.  db[n] is the same form with x = 1: the chain
 *   acc = acc + g[m,n].  M == 0 gives zeros, whatever g and x are.
 *   workspace: ps_linear_wgrad_workspace_bytes(M, N, K) bytes (0 for M <= P: then the workspace may be NULL), any alignment, not
 *   preserved between calls.  One launch for M <= P; otherwise two: the partitions' tiles into the workspace with plain stores,
 *   then the sums.  Any N, K >= 1 and any 4-byte alignment; 16-byte aligned g and x with N % 4 == 0 and K % 4 == 0 are read with
 *   16-byte requests and give the same bits.
 *   PS_EINVAL for M < 0, N < 1, K < 1, a null dW, (M > 0) a null g or x, (M > P) a null workspace; PS_EWORKSPACE for a short one.
 *
 * ps_linear_epilogue_bwd: t float[M,N] = the layer's activation after bias and ReLU and before the row norm, g float[M,N] = the
 *   gradient of the layer's output -> gz float[M,N] = the gradient of the pre-activation, one wave per row.  gz may be g.
 *   flags: a subset of PS_RELU | PS_L2NORM, any other bit PS_EINVAL.
 *   PS_L2NORM: nrm and c = max(nrm, 1e-12f) from t exactly as ps_bn_apply makes them (per-lane fmaf chain over the lane's columns
 *   64 VEC k + VEC lane + e ascending, VEC = 4 when N % 4 == 0 and t, g, gz are 16-byte aligned, else 1; the wave sum; sqrtf);
 *   y_c = t_c / c; s = sum_c g_c y_c as lane chains part = fmaf(g_c, y_c, part) from +0.0 and the same wave sum;
 *   gt_c = fmaf(-y_c, s, g_c) / c where nrm >= 1e-12f or nrm is NaN, gt_c = g_c / c below the clamp (F.normalize's clamp_min, whose
 *   gradient is zero there).  Without PS_L2NORM gt = g.
 *   PS_RELU: gz_c = t_c > 0 ? gt_c : +0.0f.  Without it gz = gt.
 *   PS_OK for M == 0, whatever the pointers; PS_EINVAL for M < 0, N < 1, (M > 0) a null g or gz, or a null t with a flag set. */
int64_t ps_linear_wgrad_partition(int64_t M);
size_t ps_linear_wgrad_workspace_bytes(int64_t M, int N, int K);
int ps_linear_wgrad(const float *g, int64_t M, int N, const float *x, int K, float *dW, float *db, void *workspace,
                    size_t workspace_bytes, ps_stream_t stream);
int ps_linear_epilogue_bwd(const float *t, const float *g, int64_t M, int N, int flags, float *gz, ps_stream_t stream);

/* ---- GraphConvLayer under loss.backward() (model/layers.py on the tape): the backward of training-mode batch norm with the layer's
 * epilogue, csrc/batch_norm_bwd.hip.  Caller-allocated buffers, no allocation, no synchronisation, no float atomics: every output
 * bit is a function of the inputs, whatever the workspace held before the call.
 *
 * ps_bn_bwd: the backward of y = epilogue(fmaf(z - mean, scale, beta)) (ps_bn_apply) where mean, var, scale float[N] are
 *   ps_bn_batch_stats' outputs for this same z float[M,N]: training-mode nn.BatchNorm1d, so the dependence of the statistics on z is
 *   part of the gradient.  gy float[M,N] is the gradient of y.  Outputs, each may be NULL (not wanted): gz float[M,N] the gradient
 *   of z, dgamma float[N], dbeta float[N] the gradients of the batch norm's weight and bias.  Nothing but z and the column vectors
 *   is read: t below is recomputed with ps_bn_apply's bits.  flags: a subset of PS_RELU | PS_L2NORM, as ps_bn_apply.
 *   Per column, fp32:   rstd = 1.0f / sqrtf(var + eps)  (sqrt and division correctly rounded).
 *   Per element, fp32:  d = z - mean (rounded); a = fmaf(d, scale, beta); t = PS_RELU ? (a < 0 ? +0 : a) : a; xh = d * rstd.
 *   Per row, PS_L2NORM only, ps_linear_epilogue_bwd's values for (t, gy): the lane chains acc = fmaf(t, t, acc) over the columns
 *     64 VEC k + VEC lane + e ascending, the wave sum, nrm = sqrtf(sum), c = max(nrm, 1e-12f); s = the wave sum of the lane chains
 *     acc = fmaf(gy, t / c, acc).  VEC = 4 when N % 4 == 0 and z, gy, gz (if given), mean, var, scale, beta are 16-byte aligned,
 *     else 1 (ps_bn_apply's rule).
 *   ga = ps_linear_epilogue_bwd's output for (t, gy, flags): nrm < 1e-12f ? gy / c : fmaf(-(t / c), s, gy) / c with PS_L2NORM, gy
 *     without; +0.0f where PS_RELU and not t > 0.
 *   Per column, fp64:   S1 = sum_r (double)ga, S2 = sum_r (double)ga * (double)xh (the product of two fp32 values is exact), in
 *     ps_bn_batch_stats' summation order: partitions of 128 consecutive rows, within a partition four strided row subsets
 *     (r0 + w, r0 + w + 4, ...) summed sequentially and added as ((s0 + s1) + s2) + s3, the partitions added ascending from 0.0.
 *   dbeta = (float)S1, dgamma = (float)S2; k1 = dbeta / (float)M, k2 = dgamma / (float)M in fp32;
 *   gz = scale * fmaf(-xh, k2, ga - k1)  (the difference rounded, then the fmaf, then the product).
 *   gz may be gy: a lane reads gy[c] for the last time before it writes gz[c].
 *   Four launches (three without PS_L2NORM, one fewer when gz is NULL): the rows' (nrm, s), the partitions' column sums, their sum
 *   with dbeta / dgamma / k1 / k2, and gz.  z and gy are read again by each; no [M, N] intermediate exists.
 *   workspace: ps_bn_bwd_workspace_bytes(M, N) bytes (0 for M < 2 or N < 1), 8-byte aligned, not preserved between calls.
 *   PS_EINVAL for M < 2, N < 1, a flag bit other than the two, a null z, gy, mean, var, scale, beta or workspace, a workspace that is
 *   not 8-byte aligned; PS_EWORKSPACE for a short one; PS_EUNSUPPORTED for M > 2^33 - 4 or more than 65 535 column
 *   blocks (N > 65 535 * 64 VEC).  Nothing is written in any of these cases.
 *   PS_OK and nothing written when all three outputs are NULL. */
size_t ps_bn_bwd_workspace_bytes(int64_t M, int N);
int ps_bn_bwd(const float *z, const float *gy, int64_t M, int N, const float *mean, const float *var, const float *scale,
              const float *beta, float eps, int flags, float *gz, float *dgamma, float *dbeta, void *workspace,
              size_t workspace_bytes, ps_stream_t stream);

/* ---- a9 (model/aggregators.py): nn.LayerNorm of ImportanceAggregator.forward with the zeroing of rows without neighbours behind it
 * (reference model/aggregators.py:213-287), both directions, csrc/layer_norm.hip.  Caller-allocated buffers, no allocation, no
 * synchronisation, no float atomics: every output bit is a function of the inputs, whatever the workspace held before the call.
 *
 * ps_layer_norm: F.layer_norm over the last dimension of x float[M,N] (dense rows) with gamma, beta float[N] -> y float[M,N], one
 *   wave per row, one launch.  VEC = 4 when N % 4 == 0 and x, y, gamma, beta are 16-byte aligned, else 1 (ps_bn_apply's rule).  A
 *   lane's columns are 64 VEC k + VEC lane + e, sweep k and element e ascending.  All arithmetic is fp32:
 *     S = the wave sum (the balanced tree of the other row kernels) of the lane chains acc = acc + x_c from +0.0; mean = S / (float)N;
 *     d_c = x_c - mean (rounded); Q = the wave sum of the lane chains acc = fmaf(d_c, d_c, acc) from +0.0; var = Q / (float)N;
 *     rstd = 1.0f / sqrtf(var + eps)  (sqrt and division correctly rounded, as ps_bn_bwd's);
 *     xh_c = d_c * rstd; y_c = fmaf(xh_c, gamma_c, beta_c).
 *   Two passes, the mean first and then the centred squares, and not E[x^2] - mean^2: a row of 100 +- 0.05 has E[x^2] = 10 000 and
 *   var = 0.0025, and one fp32 ulp of 10 000 is 0.001 -- the single-pass difference keeps no correct digit of such a variance,
 *   the centred squares keep all of them.  Rows of up to four sweeps are read once and stay in registers between the passes;
 *   longer rows are read again; both give the same bits.
 *   mean, rstd float[M]: both or neither (one alone: PS_EINVAL); ps_layer_norm_bwd reads them.
 *   live int32[M] or NULL (every row is live): row r is live iff live[r] > 0.  A dead row's x is not read; its y is +0.0 throughout
 *   and its mean[r] and rstd[r] are +0.0 (the aggregator's zeros for a node without neighbours).  A live row with a NaN is NaN
 *   throughout.  y may be x: in place gives the bits of out of place.
 *   PS_OK for M == 0, whatever the pointers; PS_EINVAL for M < 0, N < 1 or (M > 0) a null x, y, gamma or beta; PS_EUNSUPPORTED for
 *   M > 2^33 - 4 (every row has a wave of its own; grid.x holds 2^31 - 1 workgroups of four).  Nothing is written on an error.
 *
 * ps_layer_norm_bwd: the backward of the above for the same x, mean, rstd (ps_layer_norm's outputs), gamma and live; gy float[M,N] is
 *   the gradient of y.  Outputs: gx float[M,N] or NULL; dgamma, dbeta float[N], both or neither (one alone: PS_EINVAL).  VEC = 4 when
 *   N % 4 == 0 and x, gy, gx (if given), gamma are 16-byte aligned, else 1.
 *   Per element, fp32:  d = x - mean[r] (rounded); xh = d * rstd[r] (the forward's bits); gg = gy * gamma_c (rounded).
 *   Per row, fp32, the lane chains over the columns in the order above:  c1 = the wave sum of acc = acc + gg; c2 = the wave sum of
 *     acc = fmaf(gg, xh, acc); k1 = c1 / (float)N, k2 = c2 / (float)N;
 *     gx_c = rstd[r] * fmaf(-xh, k2, gg - k1)  (the difference rounded, then the fmaf, then the product: ps_bn_bwd's form transposed).
 *   A dead row: gx is +0.0, neither x nor gy is read, and the row adds nothing to the columns.
 *   Per column, fp64, over the live rows:  S1 = sum_r (double)gy, S2 = sum_r (double)gy * (double)xh (the product of two fp32 values
 *     is exact), in ps_bn_batch_stats' summation order: partitions of 128 consecutive rows of M (counted over all rows, dead or
 *     alive), within a partition four strided row subsets (r0 + w, r0 + w + 4, ...) summed sequentially and added as
 *     ((s0 + s1) + s2) + s3, the partitions added ascending from 0.0.  dbeta = (float)S1, dgamma = (float)S2.
 *   Rows in fp32, columns in fp64: a row's sums run over N terms (a few hundred) as 64 short chains and a tree, so their error is a
 *   few ulps of sum |term|; a column's run over M terms -- tens of thousands, of either sign -- where an fp32 chain would lose
 *   M 2^-24 of sum |term| against a result that cancellation makes much smaller.  The fp64 sums (exact products included) leave the
 *   one rounding to fp32 at the end.
 *   gx may be gy: the column sums are launched before the rows, and a lane reads gy[c] for the last time before it writes gx[c].
 *   Three launches: the partitions' column sums, their sum, gx; the first two only with dgamma / dbeta, the last only with gx.  With
 *   all three outputs NULL: PS_OK, nothing written.  M == 0: PS_OK, and dgamma / dbeta, if given, are set to zeros.
 *   workspace: ps_layer_norm_bwd_workspace_bytes(M, N) bytes -- 16 N bytes per partition, a function of (M, N) only, 0 for M < 1 or
 *   N < 1 -- 8-byte aligned, not preserved between calls; it may be NULL when dgamma is NULL.
 *   PS_EINVAL for M < 0, N < 1, (M > 0) a null x, gy, mean, rstd or gamma, and with dgamma a null workspace or one that is not 8-byte
 *   aligned; PS_EWORKSPACE for a short one; PS_EUNSUPPORTED for M > 2^33 - 4 or more than 65 535 column blocks (N > 65 535 * 64 VEC).
 *   Nothing is written in any of these cases. */
int ps_layer_norm(const float *x, int64_t M, int N, const float *gamma, const float *beta, float eps, const int32_t *live, float *y,
                  float *mean, float *rstd, ps_stream_t stream);
size_t ps_layer_norm_bwd_workspace_bytes(int64_t M, int N);
int ps_layer_norm_bwd(const float *x, const float *gy, int64_t M, int N, const float *mean, const float *rstd, const float *gamma,
                      const int32_t *live, float *gx, float *dgamma, float *dbeta, void *workspace, size_t workspace_bytes,
                      ps_stream_t stream);

/* One layer of the pooled branch in one call: y = epilogue( x W^T + pool(h_full) W2^T + b ), where pool(h_full) is
 * ps_importance_pool(h_full, n_full, H, ids, counts, wts, nvalid, M, T, max_idx, renorm) and the rest is ps_linear with
 * x2 = that pooled matrix (K2 = H): the same bits as that pair.  Rows that keep no neighbour skip the K2 half (their pooled row is
 * +0.0, and +0.0 * w changes no accumulator for finite w -- precondition: W2 is finite; a NaN or infinite W2 poisons such rows in
 * the pair and not here; NaN and infinities in x, h_full, W and b are carried as ps_linear carries them); the pooled rows are
 * never written as a matrix.  Served: N == 256, flags PS_RELU | PS_L2NORM (PS_WPERM allowed),
 * M >= 24 576, T <= 16, 16-byte aligned operands with K % 32 == 0 and H % 32 == 0; any other call returns PS_EUNSUPPORTED
 * without doing anything, and so does every call under the environment switch PS_GCN_FUSED=0 -- the caller then runs the pair.
 * workspace: ps_gcn_layer_workspace_bytes(M, H) bytes, 16-byte aligned, not preserved between calls.
 * Two launches: the row order (below), then the GEMM over 64-row tiles in that order. */
size_t ps_gcn_layer_workspace_bytes(int64_t M, int H);
int ps_gcn_layer(const float *x, int64_t M, int K, const float *W, int ldw, const float *b, int N, const float *h_full,
                 int64_t n_full, int H, const int32_t *ids, const int32_t *counts, const float *wts, const int32_t *nvalid,
                 int T, int64_t max_idx, int renorm, const float *W2, int ldw2, int flags, float *y, void *workspace,
                 size_t workspace_bytes, ps_stream_t stream);
/* The row order ps_gcn_layer runs its tiles in, for `layers` layers in one launch: ids int32[layers, M, T], nvalid int32[layers, M]
 * (any M >= 0, T <= 16 as in ps_gcn_layer: PS_EUNSUPPORTED otherwise).  Per layer and per chunk of 2048 consecutive rows, ord_out[2048 c ..] holds the chunk's rows that keep a neighbour
 * (j < nvalid[i], 0 <= ids[i, j] <= max_idx) in ascending order, then its other rows in ascending order; ord_out is
 * int32[layers, 64 * ceil(M / 64)], the entries from M on are -1.  tile_heavy_out int32[layers, ceil(M / 64)]: 1 where
 * ord_out[64 t .. 64 t + 63] holds a row that keeps a neighbour, else 0.  No atomics: the same output on every run.  max_idx is
 * taken as given: pass min(max_idx, n_full - 1) of the layer call.
 * ps_gcn_layer_ordered is ps_gcn_layer (same arguments, gates, workspace and results, bit for bit) with the order of its layer
 * supplied by the caller -- ord / tile_heavy: one layer's rows of the two buffers -- and is the GEMM launch alone.  The order
 * depends on the sampler's output only, so a model makes it once per step for all its layers, before the first GEMM. */
int ps_gcn_order(const int32_t *ids, const int32_t *nvalid, int layers, int64_t M, int T, int64_t max_idx, int32_t *ord_out,
                 int32_t *tile_heavy_out, ps_stream_t stream);
int ps_gcn_layer_ordered(const float *x, int64_t M, int K, const float *W, int ldw, const float *b, int N, const float *h_full,
                         int64_t n_full, int H, const int32_t *ids, const int32_t *counts, const float *wts,
                         const int32_t *nvalid, int T, int64_t max_idx, int renorm, const float *W2, int ldw2, int flags, float *y,
                         void *workspace, size_t workspace_bytes, const int32_t *ord, const int32_t *tile_heavy,
                         ps_stream_t stream);

/* ---- a10: LSHIndex.build/search (utils/nearest_neighbors.py:28-68 -> faiss.IndexLSH) ---------
 * codes[n, nbits/8] : bit j = ( x . A[j,:] >= 0 ), LSB-first (faiss fvec2bitvec); A float[nbits,D].
 * flags: 0, PS_WPERM (A stored by ps_permute_k) or PS_LSH_STAGED (A points to an image of ps_lsh_stage; not with PS_WPERM:
 * PS_EINVAL).  The same codes, bit for bit, from all three.
 *
 * ps_lsh_stage builds, once per matrix, what the staged path reads: A itself, A split into bf16 hi + lo in the order of the
 * v_mfma_f32_32x32x16_bf16 operand, and an upper bound of every row norm.  ps_lsh_encode then decides x . A[j] >= 0 from a
 * split-bf16 estimate wherever |estimate| > 2^-12 max(1, D / 256) (bound of |x|) (bound of |A[j]|), and from the exact fp32
 * fmaf chain everywhere else (zero, non-finite and out-of-range rows always) -- csrc/lsh_filter.hip.
 *   ps_lsh_stage_bytes(nbits, D) : size of the image; 0 where the staged path does not serve the shape (served: D in
 *                                  {32, 64, 128, 256} -- a wave keeps its rows' operand fragments for the whole of D in
 *                                  registers --, nbits % 32 == 0, nbits <= 1024); ps_lsh_stage / ps_lsh_encode return
 *                                  PS_EUNSUPPORTED for such shapes and for A, staged or x not 16-byte aligned.
 *   ps_lsh_stage                 : A float[nbits, D] row-major; staged_bytes below the size: PS_EINVAL.
 * Under the environment switch PS_LSH_STATS=1 a staged ps_lsh_encode adds (dots decided, dots that took the exact chain) to
 * the two uint64 counters at byte 16 of the image -- the one case in which an input is written; off by default.
 *   ps_lsh_encode_planes         : the staged ps_lsh_encode and ps_lsh_expand of its codes (below) in ONE launch: every
 *                                  workgroup also writes the sign planes of its rows, which it still holds in LDS.  staged:
 *                                  an image of ps_lsh_stage; planes: ps_lsh_planes_bytes(N, nbits / 8) bytes, all written
 *                                  (padding tiles included), equal to ps_lsh_expand(codes) bit for bit.  PS_EUNSUPPORTED
 *                                  where that size is 0 (N = 0, nbits % 64 != 0), where the staged path does not serve the
 *                                  shape and for x, staged or planes not 16-byte (codes: 4-byte) aligned; a NULL pointer is
 *                                  PS_EINVAL. */
#define PS_LSH_STAGED 8
size_t ps_lsh_stage_bytes(int nbits, int D);
int ps_lsh_stage(const float *A, int nbits, int D, void *staged, size_t staged_bytes, ps_stream_t stream);
int ps_lsh_encode(const float *x, int64_t N, int D, const float *A, int nbits, uint8_t *codes, int flags, ps_stream_t stream);
int ps_lsh_encode_planes(const float *x, int64_t N, int D, const void *staged, int nbits, uint8_t *codes, void *planes,
                         ps_stream_t stream);

/* Hamming k-NN over all codes: k smallest by (distance, id), ascending; id = row + id_offset.
 * dist int32[nq,k] (INT32_MAX pad), ids int64[nq,k] (-1 pad).  cs = bytes per code (multiple of 4). */
size_t ps_hamming_topk_workspace_bytes(int64_t nq, int64_t N, int cs, int k);
int ps_hamming_topk(const uint8_t *qcodes, int64_t nq, const uint8_t *codes, int64_t N, int cs, int k,
                    int64_t id_offset, int32_t *dist, int64_t *ids,
                    void *workspace, size_t workspace_bytes, ps_stream_t stream);

/* The same search as an exact contraction on the matrix cores (csrc/hamming_mfma.hip): every code is expanded
 * ONCE into "sign planes" -- bit j of a code -> an fp4 (e2m1) +1 / -1, laid out tile by tile (32 codes x 64 bits = 1 KiB)
 * in the order v_mfma_scale_f32_32x32x64_f8f6f4 consumes them -- and dot(q, x) = nbits - 2 * hamming(q, x) exactly (the
 * products are +-1, the partial sums integers far below 2^24).
 * Replaces the same reference lines as ps_hamming_topk (utils/nearest_neighbors.py:47-68 -> faiss hammings_knn_hc)
 * and returns bit-identical (dist, ids).
 *   ps_lsh_planes_bytes(n, cs)      : size of the plane table of n codes = 4 x the packed codes (0 if cs % 8 != 0)
 *   ps_lsh_expand(codes, n, cs, pl) : builds it (16-B aligned); done at LSHIndex.build time for the table (and per call for
 *                                     the queries by callers of ps_hamming_topk_mfma)
 *   ps_hamming_topk_mfma_codes      : the same search with the QUERIES given as packed codes (4-B aligned, cs bytes each):
 *                                     every workgroup of the scan expands its own 32 queries in registers, which saves
 *                                     the ps_lsh_expand launch in front of a search (the table's planes are still built
 *                                     once per index)
 *   ps_hamming_topk_mfma_workspace_bytes : 0 when the shape is not served (k > 32, code size not 8 / 16 / 32 / 64 bytes,
 *                                     fewer than 64 queries or 4096 items): callers use ps_hamming_topk then;
 *                                     ps_hamming_topk_mfma itself returns PS_EUNSUPPORTED for such shapes. */
size_t ps_lsh_planes_bytes(int64_t n, int cs);
int ps_lsh_expand(const uint8_t *codes, int64_t n, int cs, void *planes, ps_stream_t stream);
size_t ps_hamming_topk_mfma_workspace_bytes(int64_t nq, int64_t N, int cs, int k);
int ps_hamming_topk_mfma(const void *qplanes, int64_t nq, const void *dbplanes, int64_t N, int cs, int k,
                         int64_t id_offset, int32_t *dist, int64_t *ids,
                         void *workspace, size_t workspace_bytes, ps_stream_t stream);
int ps_hamming_topk_mfma_codes(const uint8_t *qcodes, int64_t nq, const void *dbplanes, int64_t N, int cs, int k,
                               int64_t id_offset, int32_t *dist, int64_t *ids,
                               void *workspace, size_t workspace_bytes, ps_stream_t stream);

/* Merge P sorted candidate lists per query (multi-GPU shards: all-gathered [P, nq, k]) into the
 * global k best by (distance, id). */
int ps_topk_merge(const int32_t *dist_in, const int64_t *ids_in, int P, int64_t nq, int k,
                  int32_t *dist, int64_t *ids, ps_stream_t stream);
/* The same merge over candidate lists that are not packed back to back: shard p's [nq, k] distances start at
 * dist_in + p * dist_stride, its ids at ids_in + p * ids_stride (strides in elements, >= nq * k).  Lets every rank write
 * (ids | dist) into ONE record that a single all-gather exchanges (pinsage_hip/shard.py: [P, nq*k*8 B ids | nq*k*4 B dist]). */
int ps_topk_merge_strided(const int32_t *dist_in, int64_t dist_stride, const int64_t *ids_in, int64_t ids_stride,
                          int P, int64_t nq, int k, int32_t *dist, int64_t *ids, ps_stream_t stream);

/* ---- a11: exact search (inference.py:112-118, utils/evaluation.py:106-132) --------------------
 * sim = E[q] . E^T ; optionally sim[q] = -inf ; top-k descending.  vals float[nq,k], ids int64[nq,k].  Any k >= 1
 * (k > 32: further sweeps over the similarity row, each admitting the keys after the last one emitted; k > N pads with
 * (-inf, -1)); the same holds for ps_l2_topk. */
size_t ps_dot_topk_workspace_bytes(int64_t nq, int64_t N, int D, int k);
int ps_dot_topk(const float *E, int64_t N, int D, const int64_t *qidx, int64_t nq, int k, int exclude_self,
                float *vals, int64_t *ids, void *workspace, size_t workspace_bytes, ps_stream_t stream);

/* ---- the rank of a target item (utils/evaluation.py:5-102: hit rate @ k, MRR) --------------------------------------------
 * ps_row_dot    : out[i] = A[ia[i]] . B[ib[i]], out float[n]; the arithmetic of ps_linear / ps_dot_topk (one fmaf chain, k
 *                 ascending, from +0.0), so out[i] is bit-identical to that GEMM's entry for the pair.  An index outside
 *                 [0, nA) / [0, nB) gives NaN (nothing is read).
 * ps_rank_count : E float[N,D] (the items with ids id_offset .. id_offset + N - 1), Q float[nq,D], thr float[nq], tid int64[nq]:
 *                   count[i] += #{ j in [0,N) : Q_i . E_j precedes thr[i] in ps_dot_topk's order, or equals it (same key)
 *                                               with id_offset + j < tid[i] }
 *                 ps_dot_topk's order: similarity descending by the key of its float bits (+0.0 before -0.0, NaN by bits),
 *                 ties by ascending id.  With thr[i] = ps_row_dot(Q_i, E_t) and tid[i] = t, rank = count + 1.  count int64[nq]
 *                 is ADDED to, not written: calls over disjoint item ranges (id_offset) sum to the count of their union.
 *                 One GEMM with a counting epilogue (no [nq, N] slab); N < 2^31. */
int ps_row_dot(const float *A, int64_t nA, const float *B, int64_t nB, int D, const int64_t *ia, const int64_t *ib, int64_t n,
               float *out, ps_stream_t stream);
int ps_rank_count(const float *E, int64_t N, int D, int64_t id_offset, const float *Q, int64_t nq, const float *thr,
                  const int64_t *tid, int64_t *count, ps_stream_t stream);

/* ---- two-level retrieval: exact re-rank of a first-level search's candidates -------------------------------------------------
 * The "efficient two-level retrieval" that the reference's approximate index describes (utils/nearest_neighbors.py:70-86: it
 * stores a candidates_factor and never uses it), scored as its exact search scores (inference.py:120-127): a first-level search
 * (ps_hamming_topk over LSH codes) returns R = factor * k candidate ids per query, ps_rerank_topk orders them by the exact inner
 * product.
 *   E float[N,D]: rows with the ids id_offset .. id_offset + N - 1 (as ps_hamming_topk(id_offset) emits them); Q float[nq,D];
 *   cand int64[nq,R]: one candidate list per query, as the first-level searches write it.  A candidate is valid iff
 *   0 <= id - id_offset < N; every other entry (-1 pads, ids beyond the table, negative ids) is skipped and nothing is read
 *   for it.  An id that occurs several times in a row counts once.
 *   sim = Q_i . E[id - id_offset] with ps_row_dot's arithmetic (one fmaf chain, columns ascending, from +0.0): bit-identical
 *   to the ps_linear / ps_dot_topk entry of the pair (a chain that ends in -0.0 -- every product negative and underflowing --
 *   is reported as +0.0, as the GEMM's bias addition leaves it there).
 *   vals float[nq,k], ids int64[nq,k]: the k best of the row's distinct valid candidates in ps_dot_topk's order (similarity
 *   descending by the key of its float bits, ties by ascending id), padded with (-inf, -1).
 *   k >= 1, D >= 1 (else PS_EINVAL); N < 2^31 and 1 <= R <= ps_rerank_max_candidates() (>= 4096; else PS_EUNSUPPORTED).
 *   One launch, no workspace: a query's candidate keys stay in LDS (csrc/rerank.hip). */
int ps_rerank_max_candidates(void);
int ps_rerank_topk(const float *E, int64_t N, int D, int64_t id_offset, const float *Q, int64_t nq, const int64_t *cand, int R,
                   int k, float *vals, int64_t *ids, ps_stream_t stream);

/* ---- minibatch blocks: the node set of one layer of a batch's K-hop neighbourhood (PinSage paper, Algorithm 2; the reference
 * embeds the whole catalogue, model/pinsage.py:253-280), csrc/frontier.hip.
 * ps_frontier_build: seeds int32[S] + a neighbour table ids int32[B,T] / nvalid int32[B] (ps_walk_sample's or ps_ppr_topk's)
 * -> the nodes the layer reads, the seeds first, and the table renumbered into them.  B need not equal S.
 *   Slot (i, j) is KEPT iff j < min(nvalid[i], T) and 0 <= ids[i,j] < limit: ps_importance_pool's keep rule with
 *   max_idx = limit - 1 (a negative nvalid[i] means 0, one above T means T; a slot at or beyond nvalid[i] is never kept,
 *   whatever id it holds, and no other id is used as an index).
 *   frontier int32[S + min(B * T, limit)]: the S seeds in the given order, then every kept id that is not a seed, each once,
 *   ascending.  count int32[1] = the number of entries written; the entries beyond it are left untouched.
 *   local int32[B,T]: a kept slot gets the position of its id in `frontier` (a seed's id the seed's position), every other
 *   slot -1.  S == 0: the sorted distinct kept ids, `local` the inverse map.  B == 0: the seeds alone (`local` is not touched).
 *   The seeds are distinct and lie in [0, limit).  A seed outside that range is copied to `frontier` and never used as an
 *   index; with such a seed, or one listed twice, frontier / count / local are unspecified, and every access still stays
 *   inside the buffers as sized above.
 *   Integer atomics (OR into a bitmap) and plain stores only, no float: the same inputs give the same bytes on every run,
 *   however the atomics are scheduled.
 *   PS_OK for S == 0 && B == 0 (count[0] = 0 if count is given), whatever the other pointers.  PS_EINVAL for T < 1, limit < 1,
 *   a negative S or B, limit, B * T or S + min(B * T, limit) at or above 2^31 (positions are int32), or a null pointer on a
 *   non-empty problem (seeds when S > 0; ids, nvalid, local when B > 0; frontier, count, workspace).  PS_EWORKSPACE for fewer
 *   than ps_frontier_workspace_bytes(limit, S, B, T) bytes (0 for a shape that is PS_EINVAL): two bitmaps of `limit` bits, one
 *   int32 per 32 768 ids and an int32 map of `limit` entries.  The workspace may hold anything on entry and is not preserved. */
size_t ps_frontier_workspace_bytes(int64_t limit, int64_t S, int64_t B, int T);
int ps_frontier_build(const int32_t *seeds, int64_t S, const int32_t *ids, const int32_t *nvalid, int64_t B, int T,
                      int64_t limit, int32_t *frontier, int32_t *count, int32_t *local, void *workspace,
                      size_t workspace_bytes, ps_stream_t stream);

/* ---- next row: exact L2 / IVF search behind WeakANDIndex and benchmark_search_methods
 * (utils/nearest_neighbors.py:70-139, 176: faiss.IndexFlatL2 / faiss.IndexIVFFlat).
 * dist(q, x) = |q|^2 + |x|^2 - 2 q.x in fp32; k smallest by (distance, id), ascending; dist float[nq,k]
 * (FLT_MAX pad), ids int64[nq,k] (-1 pad).  With assign int32[N] (inverted-list id of every item) and
 * probe uint32[nq, words] (bit l set = list l is probed by that query) only probed lists are visible. */
size_t ps_l2_topk_workspace_bytes(int64_t nq, int64_t N, int D, int k);
int ps_l2_topk(const float *X, int64_t N, int D, const float *Q, int64_t nq, int k, const int32_t *assign,
               const uint32_t *probe, int words, float *dist, int64_t *ids, void *workspace,
               size_t workspace_bytes, ps_stream_t stream);

/* The inverted-file form of the same scan (faiss.IndexIVFFlat, utils/nearest_neighbors.py:88-93; nprobe = min(nlist, 20), :134):
 * X float[N,D] holds the items SORTED BY LIST (list l = rows [list_ptr[l], list_ptr[l+1]), list_ptr int64[nlist+1]),
 * max_list = the longest list, item_ids int64[N] = the original id of every sorted row, probes int32[nq, nprobe] = the lists
 * each query visits (entries outside [0, nlist) are skipped).  The (query, list) pairs are grouped by list on the device,
 * one grouped fp32-MFMA product multiplies every list's queries with that list's rows only, and a query's top-k sweeps its
 * nprobe result rows: nq * nprobe * (list length) dot products instead of nq * N.  Same arithmetic per (query, item) as
 * ps_l2_topk: identical (dist, ids) to the masked form.
 * Precondition: list_ptr non-decreasing with list_ptr[0] = 0, list_ptr[nlist] = N, and max_list >= the longest list (the
 * workspace is sized from it).  A list that breaks it is clamped ON THE DEVICE to [0, N) and to max_list rows -- its tail is not
 * searched -- so no access ever leaves the workspace or X. */
size_t ps_ivf_topk_workspace_bytes(int64_t nq, int64_t N, int D, int k, int nlist, int nprobe, int64_t max_list);
int ps_ivf_topk(const float *X, int64_t N, int D, const int64_t *list_ptr, int nlist, int64_t max_list,
                const int64_t *item_ids, const float *Q, int64_t nq, const int32_t *probes, int nprobe, int k,
                float *dist, int64_t *ids, void *workspace, size_t workspace_bytes, ps_stream_t stream);

/* ---- next row: the aggregation of GraphConv.propagate (model/pinsage.py:53-54, 70-92; PyG
 * MessagePassing, aggr='add', flow source->target): out[r] = sum over the edges e of CSR row r of val[e] * x[col[e]].
 * rowptr int64[V+1] / col int32[E] = edges grouped by TARGET node (ps_csr_build with the edge_index rows swapped),
 * val float[E] = edge_weight * importance_weight in that order, or NULL (= 1); x float[N,H]; out float[V,H]
 * (rowptr[V] == E).  fp32 accumulation in edge order inside a 512-edge slice; rows cut by a slice are combined with
 * atomics, so long rows are reproducible only up to fp32 re-association, like PyG's scatter-add. */
int ps_spmm_csr(const int64_t *rowptr, const int32_t *col, const float *val, const float *x, int64_t N, int H,
                int64_t V, int64_t E, float *out, ps_stream_t stream);

/* ---- the same aggregation for training (pinsage_hip/graph.py: SpmmFn), csrc/spmm_exact.hip: an SpMM whose every output bit is a
 * function of its inputs, and the per-edge row dot that is the gradient of its edge values.  Caller-allocated buffers, no
 * allocation, no synchronisation, no float atomics.  PS_OK for an empty problem (V == 0; E == 0 zeroes out and leaves d
 * untouched), whatever the pointers; PS_EINVAL for a non-positive H, a negative size, a null pointer on a non-empty problem or a
 * short workspace; PS_EUNSUPPORTED where the grid would overflow (more than 2^31 - 1 slices).  The workspace is not preserved
 * between calls and needs no alignment.  rowptr int64[V+1] / col int32[E] as for ps_spmm_csr: rowptr[0] = 0, non-decreasing,
 * rowptr[V] = E.
 *
 * ps_spmm_csr_exact: the inputs of ps_spmm_csr (val float[E] or NULL = 1.0f, x float[N,H], out float[V,H]).
 *   Slices.  The edge slots are cut into slices [k S, (k + 1) S), S = ps_spmm_exact_slice() (a compile-time constant, 512).  The
 *   slot range [rowptr[r], rowptr[r+1]) of row r is cut by those slices into consecutive pieces.
 *   A piece is the chain acc = fmaf(val[e], x[col[e], c], acc) over its slots e ascending, from +0.0; a slot whose source id
 *   col[e] lies outside [0, N) is skipped (no operation; x is never read there).
 *   out[r, c] = ((p_0 + p_1) + p_2) + ... over the row's pieces in ascending order; p_0 alone for a row with one piece; +0.0 for
 *   an empty row.  Every element of out is written.
 *   The gradient of out with respect to x is the same entry point over the edges grouped by SOURCE node (rowptr / col = target
 *   node, val carried to that slot order) with the gradient of out as the feature matrix.
 *   workspace: ps_spmm_csr_exact_workspace_bytes(E, H) (two rows of H floats per slice; 0 for E <= 0 or H <= 0).  Two launches
 *   after a fill of out with zeros: one wave per slice (a piece that is a whole row goes straight to out, any other piece to the
 *   workspace with plain stores), then the sums of the cut rows, one wave per row.
 *
 * ps_sddmm_csr: the gradient of out with respect to val.  g float[V,H] (the gradient of out), d float[E] in CSR slot order: for
 *   slot e of row r, d[e] = sum_c g[r,c] x[col[e],c] in the arithmetic of ps_attention_bwd_rows' da: lane l chains
 *   part = fmaf(g[r,c], x[id,c], part) over its columns c = 64 VEC k + VEC l + e (sweep k and element e ascending) from +0.0, columns
 *   past H entering as 0 * 0; VEC = 4 when H % 4 == 0 and x, g are 16-byte aligned, else 1; the 64 lanes are then added by the
 *   balanced tree of ps_attention_weights (lanes 2 i and 2 i + 1 first).  A source id outside [0, N) gives +0.0 and x is not read.
 *   One launch, one wave per slice of S slots; every element of d is written. */
int ps_spmm_exact_slice(void);
size_t ps_spmm_csr_exact_workspace_bytes(int64_t E, int H);
int ps_spmm_csr_exact(const int64_t *rowptr, const int32_t *col, const float *val, const float *x, int64_t N, int H,
                      int64_t V, int64_t E, float *out, void *workspace, size_t workspace_bytes, ps_stream_t stream);
int ps_sddmm_csr(const int64_t *rowptr, const int32_t *col, const float *x, int64_t N, const float *g, int64_t V, int H,
                 int64_t E, float *d, ps_stream_t stream);

/* ---- GraphBuilder.build_item_similarity_graph (data/graph_builder.py:59-116): the item co-occurrence graph.
 * m_ua = number of rating rows (user u, item a); users are RANKS 0..U-1 in the reference's groupby('userId') order.
 * count(a, b) = sum_u m_ua m_ub (a < b), count(a, a) = sum_u m_ua (m_ua - 1) / 2: an integer GEMM A A^T over K = users,
 * contracted on the matrix cores from operand planes (csrc/cooc_mfma.hip): fp4 e2m1 when max_mult <= 4, int8 up to 127.
 *
 * ps_cooc_planes : the n distinct (user, item) entries with their multiplicity (int32 each, any order) -> planes
 *                  (ps_cooc_planes_bytes(U, M, max_mult) bytes, 16-byte aligned, zeroed here) and item_stats int64[3 M]:
 *                  [0, M) sum m (m - 1) / 2, [M, 2M) sum m^2, [2M, 3M) first user with m >= 2 (INT64 0x7f7f.. if none);
 *                  max_seen int32[1] = the largest multiplicity seen (the caller's max_mult must bound it).
 *                  max_mult > 127: PS_EUNSUPPORTED.
 * ps_cooc_pairs  : every pair a <= b < M with count >= thr (thr >= 1) as a record {a, b, count, window}; window = the
 *                  PS_COOC_WINDOW-user window that holds the first user with m_ua m_ub > 0 (m_ua >= 2 for a == b).  Records
 *                  are in no particular order.  max_sq = max over items of sum_u m_ua^2 (item_stats[M, 2M)) bounds every
 *                  count: PS_EUNSUPPORTED if it reaches 2^24 (fp4, f32 accumulation) or 2^31 (int8).  The ONE entry that
 *                  synchronises its stream: *count (device) and *h_count = the number of surviving pairs; when that exceeds
 *                  `capacity` the first `capacity` records are written and PS_EWORKSPACE is returned (rerun with more room).
 * ps_cooc_pairs_sparse : the same records as ps_cooc_pairs from the entry lists instead of planes (csrc/cooc_sparse.hip): a
 *                  row-wise sparse A A^T over the upper triangle with an LDS accumulator per item row.  No multiplicity limit,
 *                  no U x M storage, work = the reference's own pair updates.  The n distinct entries grouped by item
 *                  (iptr int64[M+1] / iuser / imult int32[n], users ascending inside an item: the arrays ps_cooc_keys takes)
 *                  and by user (eptr int64[U+1] / eitem / emult int32[n], items ascending inside a user); order int32[M] =
 *                  the item rows in the order they are handed to workgroups (a permutation of 0..M-1, heaviest row first by
 *                  sum over its users of their entry counts; any permutation gives the same records).  max_sq = max over
 *                  items of sum_u m_ua^2 bounds every count: PS_EUNSUPPORTED if it reaches 2^31 (the record's count is an
 *                  int32).  acc_slots = partners the LDS accumulator holds at once (0 = default, at most 10000); a row with
 *                  more distinct partners is redone in a global slab of M entries and stays exact.  workspace:
 *                  ps_cooc_pairs_sparse_workspace_bytes(M, acc_slots) bytes (0 = shape or acc_slots not supported; O(M) plus a
 *                  bounded number of such slabs: at most 512, at most 2 GiB but at least 4), 8-byte aligned; fewer:
 *                  PS_EWORKSPACE.  U, M < 2^31, thr >= 1, capacity >= 0, else PS_EINVAL.  Like
 *                  ps_cooc_pairs it SYNCHRONISES its stream and reports through *count / *h_count, writes the first
 *                  `capacity` records and returns PS_EWORKSPACE when there are more.
 * ps_cooc_keys   : per record the reference's dict-insertion key (u, p, q): u = the first common user, p < q the first
 *                  positions of a and b in u's group (the first two of a when a == b), as
 *                  keys[k] = (uptr[u] + p) * R + (uptr[u] + q)   (ascending key == the reference's output order).
 *                  iptr int64[M+1] / iuser int32 / imult int32: the entries grouped by item, users ascending;
 *                  uptr int64[U+1] / uitem int32[R] / upos int32[R]: the R rows grouped by user, sorted by (item, position);
 *                  upos = the row's position in its user's group (rows keep their dataframe order there).
 * ps_cooc_emit   : record perm[k] (perm int64[n], e.g. the argsort of the keys) -> edge_index int64[2, 2n] columns 2k, 2k + 1
 *                  = [a -> b, b -> a], edge_weight float[2n] = count twice. */
#define PS_COOC_WINDOW 512
typedef struct {
    int32_t a, b, count, window;
} ps_cooc_record;
size_t ps_cooc_planes_bytes(int64_t U, int64_t M, int max_mult);
int ps_cooc_planes(const int32_t *user, const int32_t *item, const int32_t *mult, int64_t n, int64_t U, int64_t M,
                   int max_mult, void *planes, size_t planes_bytes, int64_t *item_stats, int32_t *max_seen, ps_stream_t stream);
int ps_cooc_pairs(const void *planes, int64_t U, int64_t M, int max_mult, int64_t max_sq, const int64_t *item_stats, int64_t thr,
                  ps_cooc_record *records, int64_t capacity, int64_t *count, int64_t *h_count, ps_stream_t stream);
size_t ps_cooc_pairs_sparse_workspace_bytes(int64_t M, int acc_slots);
int ps_cooc_pairs_sparse(const int64_t *iptr, const int32_t *iuser, const int32_t *imult, const int64_t *eptr, const int32_t *eitem,
                         const int32_t *emult, const int32_t *order, int64_t n, int64_t U, int64_t M, int64_t max_sq, int64_t thr,
                         int acc_slots, ps_cooc_record *records, int64_t capacity, int64_t *count, int64_t *h_count,
                         void *workspace, size_t workspace_bytes, ps_stream_t stream);
int ps_cooc_keys(const ps_cooc_record *records, int64_t n, int64_t U, int64_t M, const int64_t *iptr, const int32_t *iuser,
                 const int32_t *imult, const int64_t *uptr, const int32_t *uitem, const int32_t *upos, int64_t R,
                 int64_t *keys, ps_stream_t stream);
int ps_cooc_emit(const ps_cooc_record *records, const int64_t *perm, int64_t n, int64_t *edge_index, float *edge_weight,
                 ps_stream_t stream);

/* ---- the ranking losses of model/loss.py (MaxMarginRankingLoss :6-64, BatchHardTripletLoss :66-113, CurriculumLoss :115-177):
 * loss = mean_b relu((margin + max_j Q_b . X_j) - Q_b . P_b), from one (maximum, arg-max) pair per query row.
 *
 * ps_hardest_negative : best[b] = the largest similarity Q_b . X_j and the SMALLEST j that attains it, packed in one word
 *                       (best uint64[B], 8-byte aligned, overwritten); sim float[B] / idx int64[B] (either may be NULL) receive
 *                       the pair unpacked.  flags 0: shared candidates X float[N, D] -- ps_linear's fp32-MFMA tiles with a
 *                       row-arg-max epilogue, sim[b] is bit-identical to ps_linear(Q, X)[b, idx[b]], no [B, N] slab is written;
 *                       PS_HN_EXCLUDE_DIAG: candidate j == b is left out (batch-hard: X = the positives; a row left without a
 *                       candidate gets -inf / -1).  PS_HN_PER_QUERY: X float[B, N, D], row b sees X[b] only -- the fmaf chain
 *                       of ps_row_dot, bit-identical to the shared form on equal data.  A NaN similarity is its row's maximum.
 *                       N == 0 with B > 0: PS_EINVAL.  B, N < 2^31.
 * ps_margin_loss      : with pos_b = ps_row_dot's Q_b . P_b: row_loss[b] = relu((margin + sim_b) - pos_b) (float[B], workspace),
 *                       active uint8[B] = the rows relu passes a gradient through, idx int64[B] = the arg-max, loss float[1] =
 *                       sum(row_loss) / B by a reduction of fixed shape (the same bits on every run).
 * ps_margin_loss_bwd  : g_b = grad_out[0] / B on active rows, 0 elsewhere (grad_out: DEVICE float[1]); a_b = idx[b].
 *                       dQ[b] = g_b X[a_b] + (-g_b P[b]);  dP[b] = -g_b Q[b];
 *                       PS_LOSS_PER_QUERY (X [B, N, D]): dX[b, a_b] = g_b Q[b], +0.0 elsewhere;
 *                       PS_LOSS_SHARED (X [N, D]): dX[j] = sum over {b : a_b = j, active} of g_b Q[b], b ascending;
 *                       PS_LOSS_BATCH_HARD (X = NULL, N = B, dX = NULL): X = P above and dP[j] = (-g_j Q[j]) + that sum.
 *                       Every product and sum is one rounded fp32 operation in the order written; sums over rows are taken in
 *                       ascending row order by one wave (no float atomics): deterministic.  dQ / dP / dX: NULL = not computed. */
#define PS_HN_PER_QUERY 1
#define PS_HN_EXCLUDE_DIAG 2
#define PS_LOSS_SHARED 0
#define PS_LOSS_PER_QUERY 1
#define PS_LOSS_BATCH_HARD 2
int ps_hardest_negative(const float *Q, int64_t B, int D, const float *X, int64_t N, int flags, uint64_t *best, float *sim,
                        int64_t *idx, ps_stream_t stream);
int ps_margin_loss(const float *Q, const float *P, int64_t B, int D, const uint64_t *best, float margin, float *row_loss,
                   int64_t *idx, uint8_t *active, float *loss, ps_stream_t stream);
int ps_margin_loss_bwd(const float *Q, const float *P, const float *X, int64_t B, int64_t N, int D, int mode, const int64_t *idx,
                       const uint8_t *active, const float *grad_out, float *dQ, float *dP, float *dX, ps_stream_t stream);

/* ---- personalized-PageRank neighbourhoods: RandomWalkSampler.compute_ppr_matrix (utils/random_walk.py:144-195) and
 * precompute_top_neighbors (:197-229).  All arithmetic is fp64, one rounding per product / sum / quotient, in the reference's
 * order: scores and weights are bit-identical with the reference's python floats (csrc/ppr_push.hip has the argument).
 *
 * ps_ppr_shares : share[e] = wsorted[e] / sum(row), the row sum taken left to right from 0 -- `weight / sum(w for _, w in
 *                 neighbors)` (:184).  rowptr / wsorted: ps_csr_build's; share double[E] in the same slot order.
 * ps_ppr_push   : the push sweeps (:172-188) for S sources at once.  State is node-major: score double[Vp, Sc] (overwritten),
 *                 Sc = S rounded up to 64, column s belongs to sources[s] (int64[S]; an id outside [0, Vp) stays all zero).
 *                 Vp = max(V, max(sources) + 1) as the reference sizes its vectors (:159); ids >= V have no edges.
 *                 in_rowptr int64[V+1] / in_src int32 / in_share double: the in-edges of every node IN SUMMATION ORDER -- sources
 *                 u > v ascending, then u < v ascending, multi-edges in adjacency order, self-loops left out.
 *                 level_nodes int32[V] + h_level_ptr int64[n_levels + 1] (HOST): the nodes grouped by
 *                 level(v) = 1 + max level(u) over the in-neighbours u < v; one launch per level and sweep, on `stream`.
 *                 alpha_bits: the fp64 bit pattern of alpha, 0 < alpha < 1 (the ABI carries no double scalar).
 *                 flags: PS_PPR_NO_SKIP reads every in-edge's row instead of skipping those whose 64-source slab pushed
 *                 nothing in that sweep (same result; for measurements).
 * ps_ppr_topk   : the cut of :213-227 over source-major rows score double[S, ld] (ld >= Vp): per source the k best targets with
 *                 score > 0 among ids < max_target (max_target < 0: all), score descending, ties to the smaller id.
 *                 ids int32[S, k] (-1 pad), scores double[S, k], wts double[S, k] = score / left-to-right sum in rank order
 *                 (0 pad), nvalid int32[S].
 * Precondition: edge weights are positive and finite, as ratings are.  A row whose weights sum to 0 divides by zero in the
 * reference (:184) and gives NaN shares here; negative weights give negative shares.  Neither is checked, and with such shares
 * the row skipping of ps_ppr_push (which relies on every addend being >= +0.0) need not agree with PS_PPR_NO_SKIP.
 * PS_EINVAL: k < 1, alpha outside (0, 1), negative sizes, unknown flags, a workspace smaller than
 * ps_ppr_push_workspace_bytes(Vp, S), Vp * Sc / 256 beyond 2^31 workgroups; all checked before anything is enqueued. */
#define PS_PPR_NO_SKIP 1
int ps_ppr_shares(const int64_t *rowptr, const double *wsorted, int64_t V, double *share, ps_stream_t stream);
size_t ps_ppr_push_workspace_bytes(int64_t Vp, int64_t S);
int ps_ppr_push(const int64_t *in_rowptr, const int32_t *in_src, const double *in_share, int64_t V, int64_t Vp,
                const int32_t *level_nodes, const int64_t *h_level_ptr, int n_levels, const int64_t *sources, int64_t S,
                uint64_t alpha_bits, int sweeps, int flags, double *score, void *workspace, size_t workspace_bytes,
                ps_stream_t stream);
int ps_ppr_topk(const double *score, int64_t S, int64_t ld, int64_t Vp, int64_t max_target, int k, int32_t *ids, double *scores,
                double *wts, int32_t *nvalid, ps_stream_t stream);

/* ---- hard negatives by personalized-PageRank rank (PinSage paper, section 3.3: "items ranked 2000-5000"; the reference's
 * NegativeSampler.sample_hard_negatives, data/negative_sampler.py:44-99, slices a ranking of at most 200 walked nodes, so its
 * window is always empty), csrc/rank_window.hip.
 * ps_rank_window: score double[S, ld] (ld >= Vp): source-major rows as ps_ppr_topk reads them.  limit = max_target if
 *   0 <= max_target < Vp, else Vp (ps_ppr_topk's rule).  The ranking population of row s is the ids t < limit with
 *   score[s,t] > 0 and t != skip[s] (skip int64[S]; NULL, or an entry outside [0, limit), skips nothing).  NaN, zeros of either
 *   sign and negative scores never compete; +inf does.  Columns in [limit, ld) are never candidates, columns in [Vp, ld) are
 *   never read.  Order: ps_ppr_topk's -- score descending, ties to the smaller id; ranks count from 0.
 *   window int32[S, hi - lo]: the ids whose rank r satisfies lo <= r < hi, in ASCENDING ID order (the consumer samples a set;
 *   no sort is needed), then -1 pads: the row is fully written.  nwin int32[S] = their number.  limit == 0 or a row without
 *   candidates: nwin = 0, all pads.
 *   Picks (n > 0; u double[S, n], picks int32[S, n]): Floyd's subset sampling over the window's positions.  With m = nwin[s],
 *   c = min(n, m), for i = 0 .. c-1:  j = m - c + i;  t = min((int64)floor(u[s,i] * (j + 1)), j), one fp64 product, t = 0 for a
 *   negative or NaN u;  p_i = j if t is among p_0 .. p_{i-1}, else t;  picks[s,i] = window[s, p_i].  Slots i >= c get -1.  Every
 *   c-subset of the window has the same probability under independent uniform u.  (For u < 1 the rounded product stays below
 *   j + 1, so the floor alone gives t <= j; the clamp answers a u at or above 1, infinity included.)  With n == 0,
 *   u and picks may be NULL and are not touched.
 *   One launch, one workgroup per row, no workspace: an MSB-first radix select over the 64-bit patterns of the positive scores
 *   (eight sweeps of the row, both boundaries at once), one more sweep that emits the members.  No float arithmetic decides
 *   anything but the one product above; integer LDS atomics only: the same inputs give the same bytes on every run.
 *   PS_EINVAL: negative S, Vp or n; ld < Vp; lo < 0; hi <= lo; S, Vp or hi at or above 2^31.  Then PS_OK for S == 0, nothing
 *   touched.  Then PS_EINVAL for a NULL score (with Vp > 0), window or nwin, or n > 0 with a NULL u or picks.  Then
 *   PS_EUNSUPPORTED for hi - lo > ps_rank_window_max() (65 536) or n > 64.  All checked before anything is enqueued. */
int ps_rank_window_max(void);
int ps_rank_window(const double *score, int64_t S, int64_t ld, int64_t Vp, int64_t max_target, const int64_t *skip, int64_t lo,
                   int64_t hi, const double *u, int n, int32_t *window, int32_t *nwin, int32_t *picks, ps_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* PINSAGE_HIP_H */
