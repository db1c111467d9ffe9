// rerank.hip -- the second level of a two-level search on gfx950: exact inner products of a query with ITS candidate list, and the
// k best of them in ps_dot_topk's order.
//
// The "efficient two-level retrieval" the reference describes for its approximate index (utils/nearest_neighbors.py:70-86: a
// `candidates_factor` it stores and never uses) around the exact scoring of inference.py:120-127: a first-level search
// (ps_hamming_topk over sign-LSH codes) returns R = factor * k candidate ids per query, this kernel re-ranks them.
//
// One wave per query, 64 candidates per round, lane c owns candidate c of the round.
//   gather   the candidate rows of E are fetched cooperatively, 128-byte pieces (32 columns) of 64 rows at a time: eight lanes
//            and one 16-byte request per piece, eight rows per wave-instruction, all eight instructions of a tile in flight, and
//            the next tile requested before the current one is consumed.  The query's piece travels as row 64 of the tile.  Where
//            D % 4 != 0 or a pointer is not 16-byte aligned the same tile is filled by 4-byte requests: the same floats.
//   chain    lane c runs ps_fma_chain (csrc/ps_common.h) over ITS row of the tile, piece after piece: columns ascending from
//            +0.0, one accumulator -- the bits of ps_row_dot / ps_linear / ps_dot_topk for that (query, item) pair (where the
//            chain ends in -0.0 the GEMM's +0.0, see below).  The LDS stride of 36 floats puts the 16 lanes of a ds_read_b128
//            group on 16 different 16-byte slots.
//   select   the round's keys (ps_topk_key<true>: similarity descending, ties by ascending id) go to the query's key list in
//            LDS; an invalid candidate (pad, id outside the table) leaves the empty key and nothing of E is read for it.  Then k
//            rounds of a wave minimum over "keys after the last one emitted": an id that occurs twice gives the same key twice
//            and is emitted once.
#include "ps_select.h"

namespace {

constexpr int RR_MAX_R = 4096;               // candidates per query: their keys fit in LDS beside the tile (32 KiB + 9 KiB)
constexpr int RR_DC = 32;                    // columns per tile: one 128-byte piece of every row
constexpr int RR_STRIDE = RR_DC + 4;         // floats between rows of the tile (16-byte aligned, conflict-free b128 reads)
constexpr int RR_TILE = 65 * RR_STRIDE;      // 64 candidate rows + the query's piece
constexpr int RR_LDS_MAX = 64 * 1024;        // per workgroup: the default dynamic-LDS limit, no attribute to set

__host__ __device__ inline int rr_key_slots(int R) { return (R + 1) & ~1; }                     // the tile behind stays 16-byte aligned
__host__ __device__ inline size_t rr_wave_bytes(int R) { return (size_t)rr_key_slots(R) * 8 + (size_t)RR_TILE * 4; }

template <bool VEC>
__global__ __launch_bounds__(256) void rerank_kernel(const float *__restrict__ E, int64_t N, int D, int64_t id_offset,
                                                     const float *__restrict__ Q, int64_t nq, const int64_t *__restrict__ cand,
                                                     int R, int k, float *__restrict__ vals, int64_t *__restrict__ ids) {
    extern __shared__ __attribute__((aligned(16))) unsigned char rr_lds[];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, nwv = blockDim.x >> 6;
    uint64_t *keys = reinterpret_cast<uint64_t *>(rr_lds + (size_t)wv * rr_wave_bytes(R));
    float *tile = reinterpret_cast<float *>(keys + rr_key_slots(R));
    const float *qr = tile + 64 * RR_STRIDE, *er = tile + lane * RR_STRIDE;

    for (int64_t qi = (int64_t)blockIdx.x * nwv + wv; qi < nq; qi += (int64_t)gridDim.x * nwv) {
        const float *qrow = Q + qi * D;
        for (int c0 = 0; c0 < R; c0 += 64) {
            // lane c: candidate c0 + c as a row of E, -1 = none
            int32_t ridx = -1;
            if (c0 + lane < R) {
                const int64_t id = cand[qi * R + c0 + lane];
                if (id >= id_offset && (uint64_t)id - (uint64_t)id_offset < (uint64_t)N) ridx = (int32_t)(id - id_offset);
            }
            float s = 0.f;
            if (__ballot(ridx >= 0) != 0ull) {
                if (VEC) {
                    // lane l: piece l & 7 of the rows (l >> 3) + 8 i
                    int32_t rsrc[8];
#pragma unroll
                    for (int i = 0; i < 8; ++i) rsrc[i] = __shfl(ridx, (lane >> 3) + 8 * i, 64);
                    const int pc = (lane & 7) * 4;
                    float4 buf[9];
                    auto fetch = [&](int d0) __attribute__((always_inline)) {
                        const int cols = (D - d0) < RR_DC ? (D - d0) : RR_DC;
#pragma unroll
                        for (int i = 0; i < 8; ++i) {
                            buf[i] = make_float4(0.f, 0.f, 0.f, 0.f);
                            if (rsrc[i] >= 0 && pc < cols) buf[i] = *reinterpret_cast<const float4 *>(E + (int64_t)rsrc[i] * D + d0 + pc);
                        }
                        buf[8] = make_float4(0.f, 0.f, 0.f, 0.f);
                        if (lane < 8 && pc < cols) buf[8] = *reinterpret_cast<const float4 *>(qrow + d0 + pc);
                    };
                    fetch(0);
                    for (int d0 = 0; d0 < D; d0 += RR_DC) {
                        const int cols = (D - d0) < RR_DC ? (D - d0) : RR_DC;
#pragma unroll
                        for (int i = 0; i < 8; ++i)
                            *reinterpret_cast<float4 *>(tile + ((lane >> 3) + 8 * i) * RR_STRIDE + pc) = buf[i];
                        if (lane < 8) *reinterpret_cast<float4 *>(tile + 64 * RR_STRIDE + pc) = buf[8];
                        if (d0 + RR_DC < D) fetch(d0 + RR_DC);                    // in flight under this tile's chain
                        ps_wave_lds_sync();
                        s = ps_fma_chain(qr, er, cols, true, s);
                        ps_wave_lds_sync();
                    }
                } else {
                    // lane l: column l & 31 of the rows (l >> 5) + 2 i
                    const int col = lane & 31;
                    for (int d0 = 0; d0 < D; d0 += RR_DC) {
                        const int cols = (D - d0) < RR_DC ? (D - d0) : RR_DC;
#pragma unroll 8
                        for (int i = 0; i < 32; ++i) {
                            const int row = (lane >> 5) + 2 * i;
                            const int32_t r = __shfl(ridx, row, 64);
                            if (r >= 0 && col < cols) tile[row * RR_STRIDE + col] = E[(int64_t)r * D + d0 + col];
                        }
                        if (lane < cols) tile[64 * RR_STRIDE + lane] = qrow[d0 + lane];
                        ps_wave_lds_sync();
                        const int c4 = cols & ~3;                                  // the tile's rows are 16-byte aligned whatever E is
                        s = ps_fma_chain(qr, er, c4, true, s);
                        s = ps_fma_chain(qr + c4, er + c4, cols - c4, false, s);
                        ps_wave_lds_sync();
                    }
                }
            }
            // + 0.0: the GEMM behind ps_linear / ps_dot_topk adds its absent bias as +0.0, so a chain that ends in -0.0 (every
            // product negative and underflowing) leaves it as +0.0; every other value, NaN included, is unchanged
            if (c0 + lane < R) keys[c0 + lane] = ridx >= 0 ? ps_topk_key<true>(s + 0.f, (uint32_t)ridx) : PS_EMPTY64;
        }
        ps_wave_lds_sync();

        // k rounds of "the smallest key after the last one emitted"; lane t & 63 keeps round t's key for one coalesced store
        float *vrow = vals + qi * k;
        int64_t *irow = ids + qi * k;
        uint64_t last = 0;
        bool first = true, dry = false;
        for (int t0 = 0; t0 < k; t0 += 64) {
            uint64_t mine = PS_EMPTY64;
            if (!dry) {
                const int nt = (k - t0) < 64 ? (k - t0) : 64;
                for (int u = 0; u < nt; ++u) {
                    uint64_t m = PS_EMPTY64;
                    for (int c = lane; c < R; c += 64) {
                        const uint64_t key = keys[c];
                        if ((first || key > last) && key < m) m = key;
                    }
                    const uint64_t w = ps_wave_min_u64(m);
                    if (w == PS_EMPTY64) {                                        // nothing left: the remaining slots are padding
                        dry = true;
                        break;
                    }
                    if (lane == u) mine = w;
                    last = w;
                    first = false;
                }
            }
            if (t0 + lane < k) {
                const bool some = mine != PS_EMPTY64;
                vrow[t0 + lane] = some ? ps_float_unorder(~(uint32_t)(mine >> 32)) : -INFINITY;
                irow[t0 + lane] = some ? (int64_t)(uint32_t)mine + id_offset : -1;
            }
        }
        ps_wave_lds_sync();                                                       // the next query overwrites the keys
    }
}

}  // namespace

extern "C" int ps_rerank_max_candidates(void) { return RR_MAX_R; }

extern "C" int ps_rerank_topk(const float *E, int64_t N, int D, int64_t id_offset, const float *Q, int64_t nq, const int64_t *cand,
                              int R, int k, float *vals, int64_t *ids, ps_stream_t stream) {
    if (N < 0 || D <= 0 || nq < 0 || k <= 0) return PS_EINVAL;
    if (R < 1 || R > RR_MAX_R || N > 0x7fffffff) return PS_EUNSUPPORTED;
    if (nq == 0) return PS_OK;
    if (!Q || !cand || !vals || !ids || (N > 0 && !E)) return PS_EINVAL;
    // waves (queries) per workgroup: as many of 4, 2, 1 as the key lists leave room for
    int waves = 4;
    while (waves > 1 && (size_t)waves * rr_wave_bytes(R) > (size_t)RR_LDS_MAX) waves >>= 1;
    const size_t lds = (size_t)waves * rr_wave_bytes(R);
    int64_t grid = ps_cdiv(nq, waves);
    if (grid > (1 << 20)) grid = 1 << 20;
    const bool vec = D % 4 == 0 && ps_aligned16({E, Q});
    hipStream_t st = ps_stream(stream);
    if (vec)
        hipLaunchKernelGGL(rerank_kernel<true>, dim3((unsigned)grid), dim3(64 * waves), lds, st, E, N, D, id_offset, Q, nq, cand, R, k,
                           vals, ids);
    else
        hipLaunchKernelGGL(rerank_kernel<false>, dim3((unsigned)grid), dim3(64 * waves), lds, st, E, N, D, id_offset, Q, nq, cand, R, k,
                           vals, ids);
    PS_CHECK_LAUNCH();
    return PS_OK;
}
