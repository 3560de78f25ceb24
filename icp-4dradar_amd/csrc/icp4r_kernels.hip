// icp4r_kernels.hip — the NN searches, the updates and solo_kernel, with their launches (the index build:
// icp4r_index.hip; init, the fitness prep and finish: icp4r_frame.hip).  The launch sequences are written out above
// the launch_* declarations in icp4r_internal.hpp.
#include "icp4r_fold.hpp"
#include "icp4r_tile.hpp"

namespace icp4r {

// ---------------------------------------------------------------------------------------------
// Exact brute-force 1-NN of Q register-resident queries per lane over targets [j0, j1) of a
// wave-uniform target array; increasing index order and strict '<' => lowest index wins ties.
template <int Q>
__device__ __forceinline__ void nn_sweep(const float (&x)[Q], const float (&y)[Q], const float (&z)[Q],
                                         const float4* tgt_generic, int j0, int j1, float (&best)[Q],
                                         int (&bi)[Q]) {
    const cv4f_ptr tgt = as_const(tgt_generic);
#pragma unroll
    for (int q = 0; q < Q; ++q) {
        best[q] = INFINITY;
        bi[q] = j0;
    }
    // 4 targets per trip (one s_load_dwordx16).  The last partial group re-reads target j1-1 in
    // its empty slots: a duplicate can never beat its own first occurrence under strict '<', so
    // no tail loop is needed (a tail loop — like a rotated prefetch — made hipcc keep two copies
    // of `best`, i.e. 12 instead of 11 VALU ops per pair).  Requires j1 > j0.
    const int last = j1 - 1;
    for (int j = j0; j < j1; j += 4) {
        const v4f c[4] = {tgt[j], tgt[min(j + 1, last)], tgt[min(j + 2, last)], tgt[min(j + 3, last)]};
#pragma unroll
        for (int t = 0; t < 4; ++t) {
#pragma unroll
            for (int q = 0; q < Q; ++q) {
                const float d = l2_simple(x[q], y[q], z[q], c[t].x, c[t].y, c[t].z);
                if (d < best[q]) {
                    best[q] = d;
                    bi[q] = j + t;
                }
            }
        }
    }
}

// Packed variant: two queries per v2f register pair, so the 8 arithmetic ops per pair issue as
// 4 v_pk_{add,mul}_f32 per (query-pair, target) — identical IEEE results per component (unfused,
// -ffp-contract=off) to the scalar form.  Compare/select stays scalar (no packed cmp on gfx950).
using v2f = float __attribute__((ext_vector_type(2)));

template <int Q>
__device__ __forceinline__ void nn_sweep_packed(const float (&x)[Q], const float (&y)[Q], const float (&z)[Q],
                                                const float4* tgt_generic, int j0, int j1, float (&best)[Q],
                                                int (&bi)[Q]) {
    static_assert(Q % 2 == 0, "packed sweep needs an even Q");
    constexpr int H = Q / 2;
    const cv4f_ptr tgt = as_const(tgt_generic);
    v2f px[H], py[H], pz[H];
#pragma unroll
    for (int h = 0; h < H; ++h) {
        px[h] = v2f{x[2 * h], x[2 * h + 1]};
        py[h] = v2f{y[2 * h], y[2 * h + 1]};
        pz[h] = v2f{z[2 * h], z[2 * h + 1]};
    }
#pragma unroll
    for (int q = 0; q < Q; ++q) {
        best[q] = INFINITY;
        bi[q] = j0;
    }
    const int last = j1 - 1;
    for (int j = j0; j < j1; j += 4) {
        const v4f c[4] = {tgt[j], tgt[min(j + 1, last)], tgt[min(j + 2, last)], tgt[min(j + 3, last)]};
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const v2f tx = v2f{c[t].x, c[t].x}, ty = v2f{c[t].y, c[t].y}, tz = v2f{c[t].z, c[t].z};
#pragma unroll
            for (int h = 0; h < H; ++h) {
                const v2f d0 = px[h] - tx;
                v2f r = d0 * d0;
                const v2f d1 = py[h] - ty;
                r = r + d1 * d1;
                const v2f d2 = pz[h] - tz;
                r = r + d2 * d2;
                if (r.x < best[2 * h]) {
                    best[2 * h] = r.x;
                    bi[2 * h] = j + t;
                }
                if (r.y < best[2 * h + 1]) {
                    best[2 * h + 1] = r.y;
                    bi[2 * h + 1] = j + t;
                }
            }
        }
    }
}

// Sum N doubles over a workgroup of NW waves in a fixed order (xor-butterfly per wave, then waves
// in index order by thread k for component k); totals land in `out` (LDS).
template <int N, int NW>
__device__ __forceinline__ void block_sum(double (&v)[N], double* sh /* [NW*N] */, double* out /* [N] */) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < N; ++k) v[k] = wave_sum(v[k]);
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < N; ++k) sh[wave * N + k] = v[k];
    }
    __syncthreads();
    if (threadIdx.x < N) {
        double t = 0.0;
        for (int w = 0; w < NW; ++w) t += sh[w * N + threadIdx.x];
        out[threadIdx.x] = t;
    }
    __syncthreads();
}

// Per-query NN result: one key (splits were merged by atomicMin on the key, i.e. the lexicographic
// (d², index) minimum == the unsplit sweep's answer).
__device__ __forceinline__ void load_nn(const WorkArgs& w, int64_t slot, float& d2, int& idx) {
    const NNKey k = w.nn_key[slot];
    d2 = key_d2(k);
    idx = key_idx(k);
}

// ---------------------------------------------------------------------------------------------
// nn_kernel<Q>: blockIdx.x = query block (WG*Q queries), blockIdx.y = pair, blockIdx.z = target
// split.  Writes the key of each query's nearest target in the split's index range; with several
// splits the keys are merged by a u64 atomicMin into a 0xFF..-initialised array (exact: the
// minimum key is the lexicographic (d², index) minimum, independent of arrival order).
template <int Q, bool PACKED>
__global__ __launch_bounds__(kNNWG) void nn_kernel(PairArgs a, WorkArgs w, int fitness_pass) {
    const int p = blockIdx.y;
    const int phase = uload(&w.state[p].phase);
    if (fitness_pass ? (phase == kPhaseInvalid) : (phase != kPhaseActive)) return;
    const int n = uload(a.src_n + p), m = uload(a.tgt_n + p);
    const int base = blockIdx.x * (kNNWG * Q);
    if (base >= n) return;
    const int s = blockIdx.z;
    const int j0 = (int)(((int64_t)m * s) / w.splits), j1 = (int)(((int64_t)m * (s + 1)) / w.splits);
    const float4* X = w.X + (int64_t)p * w.x_stride;
    float x[Q], y[Q], z[Q];
#pragma unroll
    for (int q = 0; q < Q; ++q) {
        const int i = base + threadIdx.x + q * kNNWG;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (i < n) v = X[i];
        x[q] = v.x;
        y[q] = v.y;
        z[q] = v.z;
    }
    float best[Q];
    int bi[Q];
    if constexpr (PACKED)
            nn_sweep_packed<Q>(x, y, z, a.tgt + uload(a.tgt_off + p), j0, j1, best, bi);
    else
        nn_sweep<Q>(x, y, z, a.tgt + uload(a.tgt_off + p), j0, j1, best, bi);
    NNKey* key = w.nn_key + (int64_t)p * w.x_stride;
    if (threadIdx.x == 0)
        count_add(w.evals, 0, (unsigned long long)(j1 - j0) * (unsigned long long)min(n - base, kNNWG * Q));
#pragma unroll
    for (int q = 0; q < Q; ++q) {
        const int i = base + threadIdx.x + q * kNNWG;
        if (i < n) {
            const NNKey k = make_key(best[q], (uint32_t)bi[q]);
            if (w.splits > 1)
                atomicMin(reinterpret_cast<unsigned long long*>(key + i), (unsigned long long)k);
            else
                key[i] = k;
        }
    }
}

// ---------------------------------------------------------------------------------------------
// nn_pruned_kernel<Q, B>: exact 1-NN with block pruning.  Each wave owns 64*Q source points that
// are contiguous in Morton order (a compact region), keeps their best key in VGPRs, and walks the
// target superblocks outward from the one holding its seed match.  A (super)block is swept only if
// some query's box lower bound can reach its current best; the sweep itself is the scalar-cache
// stream of nn_sweep with the comparison on the full (d², index) key, so the answer is exactly the
// brute-force one (PCL semantics, lowest index among ties) whatever the visiting order.
//
// Pruning is conservative in float: the bound is computed in float and shrunk by 2^-16 before the
// `<=` test, which covers the few-ulp rounding of both the bound and l2_simple's d².  Seeds: the
// previous NN of the same query (iterations > 0 and the fitness pass: the source moved by one small
// increment, so the old match is nearly as close); iteration 0: the target at the same relative
// Morton position.

// lane l's value of v, wave-uniform (v_readlane; l uniform)
__device__ __forceinline__ float rdlane(float v, int l) {
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), l));
}

template <int Q>
__device__ __forceinline__ bool box_needed(const v4f lo, const v4f hi, const float (&x)[Q], const float (&y)[Q],
                                           const float (&z)[Q], const NNKey (&best)[Q]) {
    bool need = false;
#pragma unroll
    for (int q = 0; q < Q; ++q) {
        const float gx = fmaxf(fmaxf(lo.x - x[q], x[q] - hi.x), 0.0f);
        const float gy = fmaxf(fmaxf(lo.y - y[q], y[q] - hi.y), 0.0f);
        const float gz = fmaxf(fmaxf(lo.z - z[q], z[q] - hi.z), 0.0f);
        const float lb = __builtin_fmaf(gz, gz, __builtin_fmaf(gy, gy, gx * gx));
        need = need || (lb * kLbShrink <= key_d2(best[q]));
    }
    return __any(need);
}

// Coarse (wave-uniform) test: distance between the (super)block box and the box of all the wave's
// queries against the largest best d² of the wave — a few VALU ops on uniform values instead of
// Q per-query tests; only (super)blocks that pass it get the per-query test.
__device__ __forceinline__ bool box_maybe(const v4f lo, const v4f hi, const float (&qlo)[3], const float (&qhi)[3],
                                          float qmax) {
    const float gx = fmaxf(fmaxf(lo.x - qhi[0], qlo[0] - hi.x), 0.0f);
    const float gy = fmaxf(fmaxf(lo.y - qhi[1], qlo[1] - hi.y), 0.0f);
    const float gz = fmaxf(fmaxf(lo.z - qhi[2], qlo[2] - hi.z), 0.0f);
    const float lb = __builtin_fmaf(gz, gz, __builtin_fmaf(gy, gy, gx * gx));
    return lb * kLbShrink <= qmax;
}

template <int Q, int B>
__device__ __forceinline__ void sweep_block(cv4f_ptr blk, const float (&x)[Q], const float (&y)[Q], const float (&z)[Q],
                                            NNKey (&best)[Q]) {
#pragma unroll
    for (int t = 0; t < B; t += 4) {
        const v4f c[4] = {blk[t], blk[t + 1], blk[t + 2], blk[t + 3]};
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const uint32_t ti = __float_as_uint(c[u].w);
#pragma unroll
            for (int q = 0; q < Q; ++q) {
                const NNKey kn = make_key(l2_simple(x[q], y[q], z[q], c[u].x, c[u].y, c[u].z), ti);
                best[q] = kn < best[q] ? kn : best[q];
            }
        }
    }
}

// Seed keys for the chunked pruned search (chunks > 1): every query's key := its seed evaluated at
// the query's current position — the previous match (iterations > 0 / fitness pass) or, in the
// first pass, the target at the same relative sorted position (as the unchunked kernel seeds
// inline).  The chunk searches then start from this key and merge into it with a u64 atomicMin:
// the seed is a real candidate, so min(seed, chunk minima) is the exact (d², index) minimum.
__global__ __launch_bounds__(256) void nn_seed_kernel(PairArgs a, WorkArgs w, int fitness_pass, int first) {
    const int p = blockIdx.y;
    const int phase = uload(&w.state[p].phase);
    if (fitness_pass ? (phase == kPhaseInvalid) : (phase != kPhaseActive)) return;
    const int n = uload(a.src_n + p), m = uload(a.tgt_n + p);
    const int s = blockIdx.x * 256 + threadIdx.x;
    if (s >= n) return;
    const int o = w.sperm[(int64_t)p * w.x_stride + s];
    const float4 v = w.X[(int64_t)p * w.x_stride + o];
    NNKey* key = w.nn_key + (int64_t)p * w.x_stride;
    const NNKey k0 = key[o];
    const float4* tsg = w.tsort + (int64_t)p * w.t_stride;
    uint32_t j;
    if (first && !seed_key(k0, m)) {
        j = __float_as_uint(tsg[((int64_t)s * m) / n].w);
        if (w.mo_rep) {  // a multi-workgroup Morton target: a target in the query's own cell, if any
            float lo[3], sc[3];
            mo_quant(w, p, lo, sc);
            const int32_t r = w.mo_rep[(int64_t)p * kCellBins + cell_code(v.x, v.y, v.z, lo, sc)];
            if (r >= 0 && r < m) j = (uint32_t)r;
        }
    } else {
        j = min((uint32_t)key_idx(k0), (uint32_t)(m - 1));
    }
    const float4 t = a.tgt[uload(a.tgt_off + p) + j];
    key[o] = make_key(l2_simple(v.x, v.y, v.z, t.x, t.y, t.z), j);
}

// Streamed pruned search (single pairs, small batches, targets beyond LDS — C1, C2, C5): one wave
// per 64·Q queries of a pair (Morton/kd-contiguous), blocks streamed through the scalar cache.
// grid.z = chunks: chunk c searches superblocks [c·cs, (c+1)·cs) only (cs <= 64, one lane per
// superblock for the wave's candidate mask), so a single pair fills the GPU — C5's 8 Morton chunks of
// 8192 map points, each a kd tree, or C2's target in quarters — and a wave whose query box cannot
// reach a chunk leaves after one ballot.  With chunks > 1 the seed is nn_seed_kernel's key and the
// chunk minima merge by atomicMin (correspondence records: corr_kernel afterwards).
template <int Q, int B>
__global__ __launch_bounds__(kNNWG) void nn_pruned_kernel(PairArgs a, WorkArgs w, int fitness_pass, int first, int cs) {
    const int chunks = gridDim.z, c = blockIdx.z;
    const int g = xcd_remap(blockIdx.x + gridDim.x * blockIdx.y, gridDim.x * gridDim.y);
    const int p = g / gridDim.x, qb = g - p * gridDim.x;
    const int phase = uload(&w.state[p].phase);
    if (fitness_pass ? (phase == kPhaseInvalid) : (phase != kPhaseActive)) return;
    const int n = uload(a.src_n + p), m = uload(a.tgt_n + p);
    const int nb = (m + B - 1) / B, nsb = (nb + kSuper - 1) / kSuper;
    const int sb_lo = c * cs, sb_n = min(cs, nsb - sb_lo);
    if (sb_n <= 0) return;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int base = (qb * (kNNWG / 64) + wave) * (64 * Q);
    if (base >= n) return;
    const float4* X = w.X + (int64_t)p * w.x_stride;
    const int32_t* sperm = w.sperm + (int64_t)p * w.x_stride;
    NNKey* key = w.nn_key + (int64_t)p * w.x_stride;
    const float4* tgt = a.tgt + uload(a.tgt_off + p);
    const float4* tsg = w.tsort + (int64_t)p * w.t_stride;
    float x[Q], y[Q], z[Q];
    NNKey best[Q], seed[Q];
    int orig[Q];
#pragma unroll
    for (int q = 0; q < Q; ++q) {
        const int s0 = base + lane + q * 64;
        const int s = min(s0, n - 1);  // lanes past the end repeat the last query (not written)
        const int o = sperm[s];
        orig[q] = s0 < n ? o : -1;
        const float4 v = X[o];
        x[q] = v.x;
        y[q] = v.y;
        z[q] = v.z;
        const NNKey k0 = key[o];  // chunked: nn_seed_kernel's key; else the previous key / first-pass seed
        if (chunks > 1) {
            best[q] = k0;
        } else {
            const uint32_t j = (first && !seed_key(k0, m)) ? __float_as_uint(tsg[((int64_t)s * m) / n].w)
                                                           : min((uint32_t)key_idx(k0), (uint32_t)(m - 1));
            const float4 t = tgt[j];
            best[q] = make_key(l2_simple(x[q], y[q], z[q], t.x, t.y, t.z), j);
        }
        seed[q] = best[q];
    }
    // the wave's query box and its largest seed distance (uniform; best only shrinks from here on)
    float qlo[3], qhi[3], qmax = 0.0f;
    qlo[0] = qhi[0] = x[0];
    qlo[1] = qhi[1] = y[0];
    qlo[2] = qhi[2] = z[0];
#pragma unroll
    for (int q = 0; q < Q; ++q) {
        qlo[0] = fminf(qlo[0], x[q]); qhi[0] = fmaxf(qhi[0], x[q]);
        qlo[1] = fminf(qlo[1], y[q]); qhi[1] = fmaxf(qhi[1], y[q]);
        qlo[2] = fminf(qlo[2], z[q]); qhi[2] = fmaxf(qhi[2], z[q]);
        qmax = fmaxf(qmax, key_d2(best[q]));
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {  // DPP reductions, wave-uniform results (every lane active here)
        qlo[k] = wave_minf(qlo[k]);
        qhi[k] = wave_maxf(qhi[k]);
    }
    qmax = wave_maxf(qmax);
    // the chunk's superblocks: lane l holds superblock sb_lo + l; one ballot gives the candidates
    v4f isl, ish;
    {
        const v4f* sbv = reinterpret_cast<const v4f*>(w.sbox + (int64_t)p * 2 * w.sb_stride);
        const int sbl = sb_lo + min(lane, sb_n - 1);
        isl = sbv[2 * sbl];
        ish = sbv[2 * sbl + 1];
    }
    const uint64_t cmask = __ballot(lane < sb_n && box_maybe(isl, ish, qlo, qhi, qmax));
    unsigned long long tests = (unsigned long long)sb_n;  // box tests (lane-level: one query against one box)
    int swept = 0;
    // visiting order: outward from the seed's superblock (the first lane's seed) when it lies in the
    // chunk, else from the chunk end nearest to it
    const int seed_pos = w.tinv[(int64_t)p * w.t_stride + __builtin_amdgcn_readfirstlane((uint32_t)best[0])];
    const int sb0 = __builtin_amdgcn_readfirstlane(seed_pos) / (B * kSuper) - sb_lo;
    uint64_t um = sb0 <= 0 ? cmask : sb0 < 64 ? (cmask >> sb0) << sb0 : 0ull, dm = cmask & ~um;
    const cv4f_ptr ts = as_const(tsg);
    const cv4f_ptr tb = as_const(w.tbox + (int64_t)p * 2 * w.b_stride);
    for (bool upnext = true; um | dm; upnext = !upnext) {
        int l;
        if (um && (upnext || !dm)) {
            l = __builtin_ctzll(um);
            um &= um - 1;
        } else {
            l = 63 - __builtin_clzll(dm);
            dm &= ~(1ull << l);
        }
        const v4f slo = {rdlane(isl.x, l), rdlane(isl.y, l), rdlane(isl.z, l), 0.f};
        const v4f shi = {rdlane(ish.x, l), rdlane(ish.y, l), rdlane(ish.z, l), 0.f};
        tests += 64 * Q;
        if (!box_needed<Q>(slo, shi, x, y, z, best)) continue;
        const int sb = sb_lo + l;
        for (int b = sb * kSuper; b < (sb + 1) * kSuper; ++b) {  // blocks past nb have empty boxes
            const v4f blo = tb[2 * b], bhi = tb[2 * b + 1];
            ++tests;
            if (!box_maybe(blo, bhi, qlo, qhi, qmax)) continue;
            tests += 64 * Q;
            if (!box_needed<Q>(blo, bhi, x, y, z, best)) continue;
            sweep_block<Q, B>(ts + (int64_t)b * B, x, y, z, best);
            ++swept;
        }
    }
    if (lane == 0) {
        count_add(w.evals, 0, (unsigned long long)swept * B * (unsigned long long)min(n - base, 64 * Q));
        count_add(w.evals, 1, tests);
    }
    if (chunks > 1) {  // merge; corr_kernel writes the correspondence records after every chunk
#pragma unroll
        for (int q = 0; q < Q; ++q)
            if (orig[q] >= 0 && best[q] < seed[q])
                atomicMin(reinterpret_cast<unsigned long long*>(key + orig[q]), (unsigned long long)best[q]);
        return;
    }
    if (w.corr != nullptr && !fitness_pass) {  // PCL numerics: the update's correspondence arrays
#pragma unroll
        for (int q = 0; q < Q; ++q)
            if (orig[q] >= 0) write_corr(w, a, p, orig[q], x[q], y[q], z[q], best[q], tgt);
    }
#pragma unroll
    for (int q = 0; q < Q; ++q)
        if (orig[q] >= 0) key[orig[q]] = best[q];
}

// (the batched exact 1-NN — its three launches, the search, the cached-neighbour test — is explained at the head of
// icp4r_tile.hpp, with the constants and LDS helpers of the search)
struct LdsNN {
    v4f tl[kLdsTargets];                               // 128 KB: the pair's targets, index order
    alignas(16) float bx[kLdsTargets / kLdsLeaf][6];   // 12 KB: block boxes lo.xyz, hi.xyz (empty: FLT_MAX)
    float sbx[kLdsTargets / kLdsLeaf / kSuper][6];     // 1.5 KB: superblock boxes
    union {
        unsigned long long best[kLdsWaves][64];        // 8 KB: best (d², index << 13 | position) key per query
        struct {                                       // staging: the miss bitmap and its word prefixes
            uint32_t bits[kNeedWords];
            int32_t pre[kNeedWords];
        } cz;
    } r;
    uint32_t sec[kLdsWaves][64];                       // 4 KB: second-smallest d² bits (CACHE search)
    uint16_t items[kLdsWaves][kRing + 64];             // 6 KB: (query lane << 9) | block; + a spare slot per lane
    int32_t wsum[kLdsWaves];                           // staging: bitmap popcounts per wave
    int32_t cur;                                       // (unused since claim-ahead; kept so the layout below is unchanged)
    unsigned long long selm[kLdsWaves];                // staging (reach_all): superblocks per wave's queries
    int32_t fin;                                       // (claim-ahead) waves done with their runs, all items
    int32_t nx[2][5];                                  // (claim-ahead) item k's {index, item, n, m, misses} in nx[k & 1]
};

// (lds_swz, nt_pack, lk_idx / lk_pos, write_corr_t, keys_read: icp4r_tile.hpp)

// The update that follows an NN pass clears the pair's miss bitmap and count (the next test kernel
// ORs into them; nn_light_kernel's work items all read the bitmap, so none of them can clear it).
__device__ __forceinline__ void clear_need(const WorkArgs& w, int p, int n, int tid, int nthreads) {
    if (!w.need) return;
    uint32_t* gneed = w.need + (int64_t)p * w.need_stride;
    for (int k = tid; k < (n + 31) >> 5; k += nthreads) gneed[k] = 0u;
    if (tid == 0) w.miss_cnt[p] = 0;
}

// ---- nn_cache_test_kernel: grid (chunks of kTestWG * kTestPer queries, npairs), XCD-aware.
constexpr int kTestWG = 256;
constexpr int kTestPer = 8;

__global__ __launch_bounds__(kTestWG) void nn_cache_test_kernel(PairArgs a, WorkArgs w, int fitness_pass) {
    __shared__ uint32_t need[kNeedWords];
    __shared__ int32_t wmiss[kTestWG / 64];
    __shared__ int32_t mbase;  // this workgroup's first slot in the pair's miss list
    const int chunks = gridDim.x;
    const int g = xcd_remap(blockIdx.x + chunks * blockIdx.y, chunks * gridDim.y);
    const int p = g / chunks, chunk = g - p * chunks;
    if (!pass_wants(uload(&w.state[p].phase), fitness_pass)) return;
    const int n = uload(a.src_n + p);
    const int i0 = chunk * kTestWG * kTestPer;
    if (i0 >= n) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nwords = (n + 31) >> 5;
    for (int k = tid; k < nwords; k += kTestWG) need[k] = 0;
    __syncthreads();
    float4* X = w.X + (int64_t)p * w.x_stride;
    NNKey* key = w.nn_key + (int64_t)p * w.x_stride;
    float* uu = w.nn_u + (int64_t)p * w.x_stride;
    const float4* nt = w.nn_t + (int64_t)p * w.x_stride;
    const float4* ts = w.tsort + (int64_t)p * w.t_stride;
    // In the iteration passes the previous update's transformCloud(T_inc) is applied here (the
    // update defers it: X_i is read and written once per iteration, and the bounds move with it).
    const bool xform = !fitness_pass;
    float T[16];
#pragma unroll
    for (int q = 0; q < 16; ++q) T[q] = xform ? uload(&w.state[p].T_inc[q]) : 0.0f;
    // Every load is coalesced (the NN's coordinates come from nn_t, not a gather from the target
    // cloud) and issued before the first store (a load after a store waits behind it on vmcnt).
    float4 v[kTestPer], t[kTestPer];
    float U[kTestPer];
#pragma unroll
    for (int e = 0; e < kTestPer; ++e) {
        const int i = min(i0 + e * kTestWG + tid, n - 1);
        v[e] = X[i];  // .w = L
        t[e] = nt[i];
        U[e] = uu[i];
    }
    int hits = 0, misses = 0;
    bool miss[kTestPer];
#pragma unroll
    for (int e = 0; e < kTestPer; ++e) {
        const int i = i0 + e * kTestWG + tid;
        const bool valid = i < n;
        v[e].w = fabsf(v[e].w);
        if (xform) {
            float4 o = v[e];
            xform_pt(T, v[e].x, v[e].y, v[e].z, o.x, o.y, o.z);  // PCL transformCloud, in place
            const float2 Lm = move_lu(make_float2(v[e].w, U[e]), v[e].x, v[e].y, v[e].z, o.x, o.y, o.z);
            o.w = Lm.x;
            v[e] = o;
            U[e] = Lm.y;
            if (valid) {
                X[i] = o;
                uu[i] = Lm.y;
            }
        }
        const float d2 = l2_simple(v[e].x, v[e].y, v[e].z, t[e].x, t[e].y, t[e].z);
        const bool hit = valid & cache_hit(v[e].w, d2);  // '&': a conditional use would sink the load
        const uint32_t sp = nt_pos(t[e].w);
        miss[e] = valid && !hit;
        if (hit) {
            // the finish kernel's fitness reads the keys (their d²; the index from the sorted target)
            if (keys_read(a, fitness_pass)) key[i] = make_key(d2, __float_as_uint(ts[nt_tpos(t[e].w)].w));
            ++hits;
        } else if (valid) {
            atomicOr(&need[sp >> 5], 1u << (sp & 31));
            ++misses;
        }
    }
    // this thread's misses -> slots [mbase + the workgroup's prefix, ...) of the pair's miss list
    int incl = misses;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int o = __shfl_up(incl, off, 64);
        if (lane >= off) incl += o;
    }
    if (lane == 63) wmiss[wave] = incl;
    hits = wave_sum(hits);
    if (lane == 0) {
        count_add(w.evals, 0, (unsigned long long)hits);
        count_add(w.evals, 2, (unsigned long long)hits);
        count_add(w.evals, 3, (unsigned long long)hits);
    }
    __syncthreads();
    int wbase = 0, tot = 0;
    for (int q = 0; q < kTestWG / 64; ++q) {
        wbase += q < wave ? wmiss[q] : 0;
        tot += wmiss[q];
    }
    if (tid == 0) {
        mbase = tot ? atomicAdd(w.miss_cnt + p, tot) : 0;
        count_add(w.evals, 3, (unsigned long long)tot);
    }
    __syncthreads();
    int k = mbase + wbase + incl - misses;
#pragma unroll
    for (int e = 0; e < kTestPer; ++e)
        if (miss[e]) put_miss(w, p, k++, nt_pos(t[e].w), i0 + e * kTestWG + tid, v[e].x, v[e].y, v[e].z, U[e], nt_tpos(t[e].w));
    uint32_t* gneed = w.need + (int64_t)p * w.need_stride;
    for (int q = tid; q < nwords; q += kTestWG)
        if (need[q]) atomicOr(gneed + q, need[q]);
}

// ---- nn_order_kernel: one workgroup.  Pairs to search, bucketed by floor(log2(work)) heaviest
// first (longest-processing-time-first for the persistent search; the order inside a bucket is
// arbitrary and cannot change any result).  all = 1: every pair the pass wants (first pass / no
// CACHE), work = its source count.
constexpr int kOrderWG = 1024;

__global__ __launch_bounds__(kOrderWG) void nn_order_kernel(PairArgs a, WorkArgs w, int npairs, int fitness_pass,
                                                            int all, int ncu) {
    __shared__ OrderShared sh;
    order_items<kOrderWG, false>(a, w, npairs, fitness_pass, all, ncu, sh);
}

// (RunStats, LdsTile, stage_tile, reach_all, lds_runs: icp4r_tile.hpp)

// Claim-ahead: the next work item's index, pair word, sizes and miss count are
// fetched by lane 0 of the first wave of the workgroup to finish its runs of the current item —
// three dependent round trips (the queue add, the list, the pair's sizes) that then overlap the
// slower waves' runs instead of sitting between two items.  The claim is at most one item's runs
// early (the list is heaviest first: the last items are the smallest).
__device__ __forceinline__ void claim_item(const PairArgs& a, const WorkArgs& w, int npl, int32_t* nx) {
    const int idx = atomicAdd(w.queue, 1);
    int item = 0, n = 0, m = 0, mc = 0;
    if (idx < npl) {
        item = w.plist[idx];
        const int p = item >> kPartBits;
        n = a.src_n[p];
        m = a.tgt_n[p];
        mc = w.miss_cnt ? w.miss_cnt[p] : 0;
    }
    nx[0] = idx;
    nx[1] = item;
    nx[2] = n;
    nx[3] = m;
    nx[4] = mc;
}

// ---- nn_lds_kernel<CACHE>: persistent search over the pair work list.
// CACHE: per searched query the exact second-nearest distance too, stored as the cached-neighbour
// state: L in X_i.w, U in nn_u[i], the NN's coordinates in nn_t[i] with .w = its index | the query's
// sorted position << 14 (nt_pack) — the position is what the next test flags a miss at.
// pending (launch-uniform, WorkArgs::lazy_x): the pass follows a silent tail, so the stored X of the pair's
// other points is one step behind — a searched point's L is stored with kLazyFlag (its coordinates, from
// the query record, are the moved ones in every pass).
template <bool CACHE>
__global__ __launch_bounds__(kLdsWG) void nn_lds_kernel(PairArgs a, WorkArgs w, int fitness_pass, int first, int ranked,
                                                        int pending) {
    static_assert(kLdsQ == 1, "one query per lane");
    __shared__ LdsNN sh;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const bool corr = w.corr != nullptr && !fitness_pass;
    // keys: without the cached-neighbour state the next search's seed and the records read them
    const bool want_key = !CACHE || keys_read(a, fitness_pass);
    const int npl = uload(w.plist_n);
    // work counters; debug event counters and per-phase clocks of every wave (plan option phase_ticks = 1:
    // summed over the registration in ticks[16..26], and per pass in pass_ticks[0..10];
    // tools/experiments/nn_events.py): wave-uniform adds, stored once at the end
    RunStats rs;
    if (tid == 0) {
        claim_item(a, w, npl, sh.nx[0]);
        sh.fin = 0;
    }
    __syncthreads();
    for (int it = 0;; ++it) {
        const int32_t* nx = sh.nx[it & 1];
        const int idx = __builtin_amdgcn_readfirstlane(nx[0]);
        if (idx >= npl) break;  // uniform: every wave read the same word
        const bool tk = w.ticks != nullptr && tid == 0;
        uint64_t tk0 = tk ? __builtin_amdgcn_s_memrealtime() : 0, tk1 = tk0, tk2 = tk0;
        const int item = __builtin_amdgcn_readfirstlane(nx[1]);
        const int p = item >> kPartBits, part = item & ((1 << kPartBits) - 1);
        const int n = __builtin_amdgcn_readfirstlane(nx[2]), m = __builtin_amdgcn_readfirstlane(nx[3]);
        const int nb = (m + kLdsLeaf - 1) / kLdsLeaf, nsb = (nb + kSuper - 1) / kSuper;
        const int64_t xs0 = (int64_t)p * w.x_stride;
        float4* X = w.X + xs0;
        NNKey* key = w.nn_key + xs0;
        // (the parts of a heavy pair run concurrently on other workgroups: each stages at its own
        // absolute ranks [lo, hi) and reads back from qv + lo)
        float4* qv = w.qv + xs0;
        uint2* qm = w.qm + xs0;

        // Stage the item's queries into qv / qm in list order, so every run below reads its
        // queries with one coalesced load that is issued a run ahead:
        //  * all queries (first pass / no cached state): sorted position k -> sperm[k]; X gathered,
        //    U = +inf, the seed = the target at the same relative position (or the source-order
        //    kernel's seed, or the previous key's target);
        //  * the test's misses with rank [lo, lo + part_size) (this item's part), in sorted position
        //    order: the records the test appended to the pair's miss list (sq / sm), each put at its
        //    rank in the miss bitmap.  The update kernel clears the bitmap (other parts may still be
        //    reading it).
        int nlist;
        const int mc = (CACHE && !first && ranked) ? __builtin_amdgcn_readfirstlane(nx[4]) : kMissUnranked;
        bool sel = false;  // a small ranked item: stage the superblocks its queries can reach only
        if (!(mc & kMissUnranked)) {
            // the fused test put the pair's misses in rank order already (pair_cache_test)
            const int ps = uload(w.plist_n + 2);  // the order kernel's part size for this pass
            const int lo = ps > 0 ? part * ps : 0;
            const int hi = ps > 0 ? lo + ps : (1 << 30);
            nlist = min(hi, mc) - lo;
            qv += lo;
            qm += lo;
            sel = nlist <= w.stage_sel;
        } else if (CACHE && !first) {
            const uint32_t* gneed = w.need + (int64_t)p * w.need_stride;
            const int ps = uload(w.plist_n + 2);  // the order kernel's part size for this pass
            const int lo = ps > 0 ? part * ps : 0;
            const int hi = ps > 0 ? lo + ps : (1 << 30);
            const int nwords = (n + 31) >> 5;
            const uint32_t f = tid < nwords ? gneed[tid] : 0u;
            const int c = __builtin_popcount(f);
            int incl = c;
            incl = (int)wave_scan_incl((uint32_t)incl);  // (DPP)
            if (lane == 63) sh.wsum[wave] = incl;
            __syncthreads();
            int base = 0, total = 0;
            for (int v = 0; v < kLdsWaves; ++v) {
                const int s = sh.wsum[v];
                base += v < wave ? s : 0;
                total += s;
            }
            if (tid < nwords) {
                sh.r.cz.bits[tid] = f;
                sh.r.cz.pre[tid] = base + incl - c;
            }
            nlist = min(hi, total) - lo;
            __syncthreads();
            // every record of the pair's miss list (in the test's order) goes to its rank: the
            // rank of sorted position sp = its word's prefix + the set bits below it
            const float4* sq = w.sq + xs0;
            const uint2* sm = w.sm + xs0;
            auto get = [&](int k, float4& v, uint2& mm) {
                k = min(k, total - 1);
                v = sq[k];
                mm = sm[k];
            };
            auto put = [&](int k, const float4& v, const uint2& mm) {
                const uint32_t sp = min(mm.y, (uint32_t)(n - 1));
                const int r = sh.r.cz.pre[sp >> 5] + __builtin_popcount(sh.r.cz.bits[sp >> 5] & ((1u << (sp & 31)) - 1u));
                if (k < total && r >= lo && r < hi) {
                    qv[r] = v;
                    qm[r] = make_uint2((mm.x & kNtIdxMask) | (sp << kNtPosShift), mm.x >> kNtPosShift);
                }
            };
#pragma nounroll
            for (int k0 = tid; k0 < total; k0 += 4 * kLdsWG) {
                float4 v0, v1, v2, v3;  // (named, not an array: an array here went to scratch)
                uint2 m0, m1, m2, m3;
                get(k0, v0, m0);  // all loads of the round issued together
                get(k0 + kLdsWG, v1, m1);
                get(k0 + 2 * kLdsWG, v2, m2);
                get(k0 + 3 * kLdsWG, v3, m3);
                put(k0, v0, m0);
                put(k0 + kLdsWG, v1, m1);
                put(k0 + 2 * kLdsWG, v2, m2);
                put(k0 + 3 * kLdsWG, v3, m3);
            }
            qv += lo;  // this item's slice, read back by the runs
            qm += lo;
        } else if (first && w.stage_first && src_by_tgt_tree(a, w, p)) {
            nlist = n;  // src_order_kernel wrote the records
        } else {
            const int32_t* sperm = w.sperm + xs0;
            const int32_t* tinv = w.tinv + (int64_t)p * w.t_stride;
            for (int k0 = 0; k0 < n; k0 += 4 * kLdsWG) {
                int o[4];
                float4 v[4];
                NNKey pk[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) o[e] = sperm[min(k0 + e * kLdsWG + tid, n - 1)];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    v[e] = X[o[e]];
                    pk[e] = key[o[e]];
                }
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int k = k0 + e * kLdsWG + tid;
                    if (k >= n) continue;
                    // seed: the previous match (no cached state), the source-order kernel's leaf, or
                    // the target at the same relative position
                    const bool prev = !first || seed_key(pk[e], m);
                    const int seed = prev ? tinv[min((uint32_t)key_idx(pk[e]), (uint32_t)(m - 1))]
                                          : (int)(((int64_t)k * m) / n);
                    qv[k] = make_float4(v[e].x, v[e].y, v[e].z, INFINITY);
                    qm[k] = make_uint2((uint32_t)o[e] | ((uint32_t)k << kNtPosShift), (uint32_t)seed);
                }
            }
            nlist = n;
        }
        if (tk) tk1 = __builtin_amdgcn_s_memrealtime();

        // Stage the pair's sorted targets into LDS (.w = original index << 13 | position) and the block
        // and superblock boxes, and load every lane's superblock box (isl / ish: lane l holds
        // superblock l's box for every run of the item; nsb <= 64 on this plan).  Every load is issued
        // before the first store: a load-store loop waited out one global round trip per target
        // (8 per thread, ~10-20 us per item under load).
        const LdsTile tv{sh.tl, sh.bx, sh.sbx};
        v4f isl, ish;
        const uint64_t M = sel ? reach_all<kLdsWG>(sh.selm, w, p, nsb, m, qv, qm, nlist) : ~0ull;
        stage_tile<kLdsWG>(tv, w, p, nsb, isl, ish, M);
        __syncthreads();  // LDS targets; qv / qm (global, this workgroup's) visible to every wave
        if (tk) tk2 = __builtin_amdgcn_s_memrealtime();
        unsigned long long* bestl = sh.r.best[wave];
        uint32_t* secl = sh.sec[wave];
        uint16_t* ring = sh.items[wave];
        lds_runs<CACHE>(tv, bestl, secl, ring, qv, qm, nlist, m, nsb, isl, ish, a, w, p, xs0, X, key, want_key, corr, rs,
                        pending ? kLazyFlag : 0u);
        // the first wave done claims the next item (sh.nx[(it + 1) & 1]: item it - 1's words, read by
        // every wave before this item's staging barrier)
        if (lane == 0 && atomicAdd(&sh.fin, 1) == it * kLdsWaves) claim_item(a, w, npl, sh.nx[(it + 1) & 1]);
        __syncthreads();  // LDS (targets, per-wave state) is reused by the next pair
        if (tk) {
            unsigned long long* tt = reinterpret_cast<unsigned long long*>(w.ticks);
            atomicAdd(tt + 8, (unsigned long long)(tk1 - tk0));
            atomicAdd(tt + 9, (unsigned long long)(tk2 - tk1));
            atomicAdd(tt + 10, (unsigned long long)(__builtin_amdgcn_s_memrealtime() - tk2));
            atomicAdd(tt + 11, 1ull);
            if (w.pass_ticks) {  // the same walls in this pass' own slots
                unsigned long long* pt = reinterpret_cast<unsigned long long*>(w.pass_ticks);
                atomicAdd(pt + 11, (unsigned long long)(tk1 - tk0));
                atomicAdd(pt + 12, (unsigned long long)(tk2 - tk1));
                atomicAdd(pt + 13, (unsigned long long)(__builtin_amdgcn_s_memrealtime() - tk2));
                atomicAdd(pt + 14, 1ull);
            }
        }
    }
    if (lane == 0) {
        count_add(w.evals, 0, rs.evals);
        count_add(w.evals, 1, rs.tests);
        if (w.ticks) {
            unsigned long long* tt = reinterpret_cast<unsigned long long*>(w.ticks);
            const unsigned long long ev[11] = {rs.ev_runs, rs.ev_q,     rs.ev_sbv,   rs.ev_sbp,  rs.ev_blk,  rs.ev_push,
                                               rs.ev_drain, rs.ev_items, rs.ck_setup, rs.ck_trav, rs.ck_write};
            for (int k = 0; k < 11; ++k) atomicAdd(tt + 16 + k, ev[k]);
            if (w.pass_ticks)
                for (int k = 0; k < 11; ++k) atomicAdd(reinterpret_cast<unsigned long long*>(w.pass_ticks) + k, ev[k]);
        }
    }
}

// ---------------------------------------------------------------------------------------------
// nn_tile_kernel: the pruned plan's search (single pairs, small batches, targets of any size — the
// C1 / C2 pairs and the C5 scan-to-map target) with the batched search's LDS machinery.  Grid:
// (target tiles of kLdsTargets sorted positions, query parts of kLdsWG sorted sources, pairs).  A
// workgroup stages its tile (targets and block / superblock boxes) in LDS and searches its queries
// against it, one query per lane in runs of 64 consecutive sorted sources: the tile's superblocks
// tested against the run's box at once, a reached superblock's 8 blocks tested for every lane, the
// non-empty (lane, block) items queued per wave and drained 64 at a time (16 targets from LDS per
// lane).  A query starts from its current key — nn_seed_kernel's seed, or another tile's minimum read
// at the start (any key read is an upper bound: keys only fall) — and merges its tile minimum into it
// with a u64 atomicMin (exact: the lexicographic (d², index) minimum whatever the order of tiles).
// corr_kernel writes the correspondence records afterwards.  Replaces the scalar-cache stream of
// nn_pruned_kernel, whose every block visit evaluated the block for all 64 lanes of a wave.
struct TileShared {
    v4f tl[kLdsTargets];                              // 128 KB: the tile's targets (.w = index << 13 | position)
    alignas(16) float bx[kLdsTargets / kLdsLeaf][6];  // block boxes (empty: FLT_MAX)
    float sbx[kLdsTargets / kLdsLeaf / kSuper][6];    // superblock boxes
    unsigned long long best[kLdsWaves][64];           // per query: best local key
    uint16_t items[kLdsWaves][kRing + 64];            // (query lane << 9) | block; + a spare slot per lane
};
constexpr int kTileMaxM = 1 << (32 - kLdsPosBits);  // target indices that fit the local key

//
// One tile (every target of the pass fits one tile: C1, C2), `first` >= 0: the workgroup owns its
// queries' whole search, so the seed (the previous match; first pass: the target at the same
// relative sorted position — nn_seed_kernel's rule) is evaluated here, the key is stored, not merged,
// and the correspondence record is written from the winner's LDS slot — one launch per NN pass
// instead of three (seed, search, records), two kernel boundaries fewer per ICP iteration.
__global__ __launch_bounds__(kLdsWG) void nn_tile_kernel(PairArgs a, WorkArgs w, int fitness_pass, int first, int qrun) {
    __shared__ TileShared sh;
    const bool own = first >= 0;  // (single tile: launched with gridDim.x == 1)
    const int tile = blockIdx.x, part = blockIdx.y, p = blockIdx.z;
    const unsigned long long tk_entry = w.pass_ticks ? __builtin_amdgcn_s_memrealtime() : 0;
    const int phase = uload(&w.state[p].phase);
    if (fitness_pass ? (phase == kPhaseInvalid) : (phase != kPhaseActive)) return;
    const int n = uload(a.src_n + p), m = uload(a.tgt_n + p);
    const int t0 = tile * kLdsTargets, q0 = part * kLdsWaves * qrun;  // (qrun queries per wave: 64, 32, 16, 8)
    if (t0 >= m || q0 >= n) return;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int tm = min(kLdsTargets, m - t0);
    const int nb = (tm + kLdsLeaf - 1) / kLdsLeaf, nsb = (nb + kSuper - 1) / kSuper;
    const int64_t xs0 = (int64_t)p * w.x_stride;
    unsigned long long evals = 0, tests = 0;
    // debug (plan option phase_ticks = 1): workgroup (0, 0, 0)'s stamps in the pass' slots 0..4, and
    // over every workgroup the earliest start (slot 6, as its complement) and the latest end (slot 5)
    unsigned long long* tk = (w.pass_ticks && tid == 0) ? reinterpret_cast<unsigned long long*>(w.pass_ticks) : nullptr;
    const bool tk0 = tk && tile == 0 && part == 0 && p == 0;
    const unsigned long long tk_in = tk ? __builtin_amdgcn_s_memrealtime() : 0;
    if (tk0) tk[0] = tk_in;
    if (tk0) tk[7] = tk_entry;
    if (tk) atomicMax(tk + 6, ~tk_in);

    // Stage the tile (whole superblocks: tsort is padded to them), every load before the first store,
    // with the query's chain of dependent loads beside it: the query's sorted position goes out first,
    // then the tile, then its point and key (behind the position only: the tile's loads stay in
    // flight), the seed target, and the tile's LDS stores while that last load is out.  (The chain had
    // started after the staging barrier: ~1.2 us of a 2k pass' 5.4 per workgroup; behind the tile's
    // loads it would wait for them at its first step.)
    const int r0 = q0 + wave * qrun;  // this wave's run: sorted sources [r0, r0 + qrun)
    const bool wrun = r0 < n;         // (wave-uniform)
    const bool live = wrun && lane < qrun && r0 + lane < n;
    const int sq = live ? r0 + lane : min(r0, n - 1);
    // (unconditional loads, clamped: a load under a branch merges into a copy that waits for it)
    const int o = w.sperm[xs0 + sq];  // idle lanes shadow the run's first query
    __builtin_amdgcn_sched_barrier(0);  // (the order of issue above and below is the point)
    const v4f* tsg = reinterpret_cast<const v4f*>(w.tsort + (int64_t)p * w.t_stride + t0);
    const v4f* tb = reinterpret_cast<const v4f*>(w.tbox + (int64_t)p * 2 * w.b_stride) + 2 * (t0 / kLdsLeaf);
    const v4f* sbg = reinterpret_cast<const v4f*>(w.sbox + (int64_t)p * 2 * w.sb_stride) + 2 * (t0 / (kLdsLeaf * kSuper));
    const int nt = nsb * kSuper * kLdsLeaf;
    constexpr int kPerT = kLdsTargets / kLdsWG;
    v4f tv[kPerT];
#pragma unroll
    for (int k = 0; k < kPerT; ++k) tv[k] = tsg[min(tid + k * kLdsWG, nt - 1)];
    const int nbx = nsb * (kSuper + 1);
    const int bq = min(tid, nbx - 1);
    const bool blk = bq < nsb * kSuper;
    const int bk = blk ? bq : bq - nsb * kSuper;
    const v4f blo = blk ? tb[2 * bk] : sbg[2 * bk], bhi = blk ? tb[2 * bk + 1] : sbg[2 * bk + 1];
    const int sbl = min(lane, nsb - 1);
    const v4f isl = sbg[2 * sbl], ish = sbg[2 * sbl + 1];
    __builtin_amdgcn_sched_barrier(0);

    unsigned long long* bestl = sh.best[wave];
    uint16_t* ring = sh.items[wave];
    NNKey* key = w.nn_key + xs0;
    float x = 0.f, y = 0.f, z = 0.f;
    NNKey init = 0;
    // the fitness pass with w.fit_xform (own plans): the query is final * input_i, formed here as
    // fitness_prep_kernel did (Registration::getFitnessScore's transformPointCloud) and written to X
    const bool fitx = own && fitness_pass && w.fit_xform;
    float4 v = fitx ? a.src[uload(a.src_off + p) + o] : w.X[xs0 + o];
    NNKey k0 = key[o];
    uint32_t j = 0;
    float4 t;
    {
        if (fitx) {
            float T[16];
#pragma unroll
            for (int q = 0; q < 16; ++q) T[q] = uload(&w.state[p].final_T[q]);
            xform_pt(T, v.x, v.y, v.z, v.x, v.y, v.z);
            if (live) w.X[xs0 + o] = v;
        }
        if (own && first == 0 && !fitness_pass && w.defer_xform) {
            // the previous update's transformCloud(T_inc), deferred to here (one read and write of X
            // per pass instead of a pass over the cloud by the update's one workgroup); every query
            // belongs to one lane of one workgroup of the single tile, which writes it back
            float T[16];
#pragma unroll
            for (int q = 0; q < 16; ++q) T[q] = uload(&w.state[p].T_inc[q]);
            xform_pt(T, v.x, v.y, v.z, v.x, v.y, v.z);
            if (live) w.X[xs0 + o] = v;
        }
        x = v.x;
        y = v.y;
        z = v.z;
        // the seed (nn_seed_kernel's rule, own: evaluated at the query's current position); loaded on
        // every plan for the same reason (the multi-tile plan does not use it)
        j = (own && first && !seed_key(k0, m)) ? __float_as_uint(w.tsort[(int64_t)p * w.t_stride + ((int64_t)sq * m) / n].w)
                                               : min((uint32_t)key_idx(k0), (uint32_t)(m - 1));
        t = a.tgt[uload(a.tgt_off + p) + j];
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int k = 0; k < kPerT; ++k) {
        const int i = tid + k * kLdsWG;
        if (i < nt) {
            sh.tl[lds_swz(i)] = tl_slot(tv[k], (__float_as_uint(tv[k].w) << kLdsPosBits) | (uint32_t)i);
        }
    }
    if (tid < nbx) {
        const bool empty = !(blo.x <= bhi.x);
        float* d = blk ? sh.bx[bk] : sh.sbx[bk];
        d[0] = empty ? FLT_MAX : blo.x; d[1] = empty ? FLT_MAX : blo.y; d[2] = empty ? FLT_MAX : blo.z;
        d[3] = empty ? FLT_MAX : bhi.x; d[4] = empty ? FLT_MAX : bhi.y; d[5] = empty ? FLT_MAX : bhi.z;
    }
    __builtin_amdgcn_sched_barrier(0);
    if (wrun) {
        if (own) k0 = make_key(l2_simple(x, y, z, t.x, t.y, t.z), j);
        // the current key in the tile's encoding, ranked after every real target of the same (d², index)
        init = make_key(key_d2(k0), ((uint32_t)key_idx(k0) << kLdsPosBits) | ((1u << kLdsPosBits) - 1));
        bestl[lane] = init;  // (sh.best: not staged)
    }
    if (tk0) tk[2] = __builtin_amdgcn_s_memrealtime();
    __syncthreads();
    if (tk0) tk[1] = __builtin_amdgcn_s_memrealtime();
    if (!wrun) return;  // (no barrier follows)
    float bnd = live ? key_d2(k0) * kLbGrow : -1.0f;
    float qlo[3] = {x, y, z}, qhi[3] = {x, y, z};
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        qlo[k] = wave_minf(qlo[k]);
        qhi[k] = wave_maxf(qhi[k]);
    }
    const float qmax = wave_maxf(bnd);
    const uint32_t lane9 = (uint32_t)lane << 9;
    uint32_t head = 0, tail = 0;
    auto drain = [&](uint32_t cnt) {
        const bool act = (uint32_t)lane < cnt;
        const uint32_t it = ring[(head + lane) & (kRing - 1)];
        const int owner = act ? (int)(it >> 9) : 0;
        const int b = act ? (int)(it & 0x1ffu) : 0;
        const float qx = __shfl(x, owner, 64), qy = __shfl(y, owner, 64), qz = __shfl(z, owner, 64);
        if (act) {
            NNKey k1 = ~0ull;
            v4f cs[kLdsLeaf];
            lds_block(sh.tl, b, cs);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int t = 0; t < kLdsLeaf; ++t) {
                const v4f c = cs[t];
                const NNKey kn = make_key(l2_simple(qx, qy, qz, tl_x(c), tl_y(c), tl_z(c)), tl_key(c));
                k1 = kn < k1 ? kn : k1;
            }
            atomicMin(&bestl[owner], k1);
        }
        head += cnt;
        evals += (unsigned long long)cnt * kLdsLeaf;
        bnd = live ? key_d2(bestl[lane]) * kLbGrow : -1.0f;
    };
    // the tile's superblocks some query may reach, visited in order (the run's neighbourhood is
    // unknown here: no seed inside the tile)
    uint64_t cm = __ballot(lane < nsb && box_lb(isl, ish, qlo, qhi) <= qmax);
    tests += nsb;
    for (; cm; cm &= cm - 1) {
        const int sb = __builtin_ctzll(cm);
        const auto* sbb = lds_vbase(&sh.sbx[sb][0]);
        tests += 64;
        if (__ballot(pt_lb(sbb, x, y, z) <= bnd) == 0) continue;
        uint64_t nmk[kSuper];
#pragma unroll
        for (int h = 0; h < kSuper; h += 4) {
            const auto* b4 = (const __attribute__((address_space(3))) v4f*)lds_vbase(&sh.bx[sb * kSuper + h][0]);
            v4f r4[6];
#pragma unroll
            for (int i = 0; i < 6; ++i) r4[i] = b4[i];
            float bb[4][6];
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int c = 0; c < 6; ++c) bb[j][c] = r4[(6 * j + c) >> 2][(6 * j + c) & 3];
#pragma unroll
            for (int j = 0; j < 4; ++j) nmk[h + j] = __ballot(pt_lb(bb[j], x, y, z) <= bnd);
        }
        tests += 64 * kSuper;
#pragma unroll
        for (int k = 0; k < kSuper; ++k) {
            const uint64_t mask = nmk[k];
            if (mask == 0) continue;
            const uint32_t slot = __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32),
                                                            __builtin_amdgcn_mbcnt_lo((uint32_t)mask, tail));
            const uint32_t at = lane_select(mask, (uint32_t)(kRing + lane), slot & (kRing - 1));
            ring[at] = (uint16_t)(lane9 | (uint32_t)(sb * kSuper + k));
            tail += (uint32_t)__builtin_popcountll(mask);
            if (tail - head >= 64) drain(64);
        }
    }
    if (tail != head) drain(tail - head);
    const NNKey kb = bestl[lane];
    if (tk0) tk[3] = __builtin_amdgcn_s_memrealtime();
    if (own) {
        // the seed target lies in the tile and its block's bound cannot prune it, so the winner is a
        // real LDS slot; the sentinel position (kb == init) is handled all the same
        const NNKey ko = kb < init ? make_key(key_d2(kb), lk_idx(kb)) : k0;
        if (live) {
            key[o] = ko;
            if (w.corr != nullptr && !fitness_pass) {  // PCL numerics: the update's correspondence records
                const float4 t = kb < init ? [&] {
                    const v4f c = sh.tl[lds_swz((int)lk_pos(kb))];
                    return make_float4(tl_x(c), tl_y(c), tl_z(c), 0.f);
                }() : a.tgt[uload(a.tgt_off + p) + key_idx(k0)];
                write_corr_t(w, a, p, o, x, y, z, key_d2(ko), t);
            }
        }
    } else if (live && kb < init) {
        atomicMin(&key[o], make_key(key_d2(kb), lk_idx(kb)));
    }
    if (lane == 0) {
        count_add(w.evals, 0, evals);
        count_add(w.evals, 1, tests);
    }
    if (tk) {
        const unsigned long long t = __builtin_amdgcn_s_memrealtime();
        if (tk0) tk[4] = t;
        atomicMax(tk + 5, t);
    }
}

// Brute-force path: the correspondence arrays from the merged NN keys (the pruned kernel writes
// them itself).
__global__ __launch_bounds__(256) void corr_kernel(PairArgs a, WorkArgs w) {
    const int p = blockIdx.y;
    if (uload(&w.state[p].phase) != kPhaseActive) return;
    const int n = uload(a.src_n + p);
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float4 s = w.X[(int64_t)p * w.x_stride + i];
    write_corr(w, a, p, i, s.x, s.y, s.z, w.nn_key[(int64_t)p * w.x_stride + i], a.tgt + uload(a.tgt_off + p));
}

// ---------------------------------------------------------------------------------------------
// The 3x3 solve and convergence test of one pair (thread 0), shared by both numerics.
struct SolveShared {
    double mom[20];
    double sigma[9], ms[3], md[3];
    SvdWork svd;
    float sigmaf[9];  // PCL numerics: sigma as Eigen's GEMM leaves it (one_over_n applied per panel)
    float mean[6];
    float one_over_n;
    int32_t bnd[16];  // pass B with rejected correspondences: the group's panel starts (point index)
    int32_t wsum[16];  // (its scan's per-wave counts)
    double mse_sum;
    float T_inc[16];
    int32_t flag;  // 0 continue, 1 error (no transform), 2 converged after this transform
};

template <int NUM> struct MomLayout;
template <> struct MomLayout<kNumericsPCL> {  // |C| only: every other sum is a sequential fold
    static constexpr int N = 1, CNT = 0;
};
template <> struct MomLayout<kNumericsF64> {  // Σ w·d·sᵀ [9], Σ w·s [3], Σ w·d [3], Σ w, Σ d², |C|
    static constexpr int N = 18, MSE = 16, CNT = 17;
};

// (solve_pair_body: always inlined — fold_update_res_kernel keeps its pair in registers across the solve,
// and a call would spill every caller-saved one of them; solve_pair: the other kernels' call)
template <int NUM>
__device__ __forceinline__ void solve_pair_body(SolveShared& sh, PairState& st, const KParams& kp) {
    constexpr int I_CNT = MomLayout<NUM>::CNT;
    const int cnt = (int)sh.mom[I_CNT];
    st.ncorr = cnt;
    if (cnt < kp.min_corr) {
        // PCL_ERROR "Not enough correspondences found. Relax your threshold parameters."
        st.phase = kPhaseFailed;
        st.status = kStatusTooFewCorr;
        st.conv_state = 5;  // CONVERGENCE_CRITERIA_NO_CORRESPONDENCES
        sh.flag = 1;
        return;
    }
    // the pair state this serial solve reads, loaded up front (in flight during the SVD): each had
    // been a dependent global load on thread 0's critical path
    float F[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) F[k] = st.final_T[k];
    ConvState cs;
    cs.prev_mse = st.prev_mse;
    cs.similar = st.similar;
    cs.state = st.conv_state;
    const int32_t iters = st.iterations + 1;
    float* Tinc = sh.T_inc;
    mat4_identity(Tinc);
    double mse;
    if constexpr (NUM == kNumericsPCL) {
        // Eigen umeyama, Scalar = float: sigma = one_over_n * Σ d' s'ᵀ (fold_pass_b: Eigen's blocked
        // GEMM, already scaled), float SVD, R as Matrix4f, Rt.col(3) = dst_mean; Rt.col(3) -= R * src_mean.
        // (in registers: umeyama_rotation_f32_reg is umeyama_rotation_f32 with static indices)
        float sg[9], R[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) sg[k] = sh.sigmaf[k];
        umeyama_rotation_f32_reg(sg, R);
#pragma unroll
        for (int i = 0; i < 3; ++i) {
#pragma unroll
            for (int j = 0; j < 3; ++j) Tinc[j * 4 + i] = R[i * 3 + j];
            float rs = R[i * 3 + 0] * sh.mean[0];
            rs = R[i * 3 + 1] * sh.mean[1] + rs;
            rs = R[i * 3 + 2] * sh.mean[2] + rs;
            Tinc[12 + i] = sh.mean[3 + i] - rs;
        }
        mse = sh.mse_sum / (double)cnt;  // calculateMSE: sequential double sum / |C|
    } else {
        const double sw = sh.mom[15];
        for (int k = 0; k < 3; ++k) {
            sh.ms[k] = sh.mom[9 + k] / sw;
            sh.md[k] = sh.mom[12 + k] / sw;
        }
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) sh.sigma[i * 3 + j] = sh.mom[i * 3 + j] / sw - sh.md[i] * sh.ms[j];
        umeyama_rotation(sh.sigma, sh.svd);
        const double* R = sh.svd.R;
        for (int i = 0; i < 3; ++i) {
            for (int j = 0; j < 3; ++j) Tinc[j * 4 + i] = (float)R[i * 3 + j];
            Tinc[12 + i] = (float)(sh.md[i] - (R[i * 3 + 0] * sh.ms[0] + R[i * 3 + 1] * sh.ms[1] + R[i * 3 + 2] * sh.ms[2]));
        }
        mse = sh.mom[MomLayout<kNumericsF64>::MSE] / (double)cnt;
    }
    for (int k = 0; k < 16; ++k) st.T_inc[k] = Tinc[k];
    float Fn[16];
    mat4_mul_f(Tinc, F, Fn);  // final_transformation_ = transformation_ * final
#pragma unroll
    for (int k = 0; k < 16; ++k) st.final_T[k] = Fn[k];
    st.iterations = iters;
    const int conv = has_converged(kp.conv, iters, Tinc, mse, cs);
    st.prev_mse = cs.prev_mse;
    st.similar = cs.similar;
    st.conv_state = cs.state;
    if (conv) st.phase = kPhaseConverged;
    sh.flag = conv ? 2 : 0;
}
template <int NUM>
__device__ void solve_pair(SolveShared& sh, PairState& st, const KParams& kp) {
    solve_pair_body<NUM>(sh, st, kp);
}

// transformCloud(*input_transformed, *input_transformed, transformation_) by the whole workgroup.
// (With the cached-neighbour test the update defers this to the next pass's test kernel.)
// seed (w.seed_next): the next NN pass's starting key too — the current NN (its coordinates from the
// correspondence record, its index from the key) at the moved point, as nn_seed_kernel computes it.
template <int WG>
__device__ __forceinline__ void transform_pair(const WorkArgs& w, int p, int n, const float* T_lds, bool seed) {
    float Tl[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) Tl[k] = T_lds[k];
    const int64_t xs0 = (int64_t)p * w.x_stride;
    float4* X = w.X + xs0;
    NNKey* key = w.nn_key + xs0;
    const float4* C = w.corr + xs0 * 2;
    // kPer points per thread with every load in flight before the first store (a load issued after a
    // store waits behind it on vmcnt: one L2 round trip per point otherwise)
    constexpr int kPer = 4;
    for (int i0 = 0; i0 < n; i0 += WG * kPer) {
        float4 s[kPer], t[kPer];
        NNKey k0[kPer];
#pragma unroll
        for (int e = 0; e < kPer; ++e) {
            const int i = min(i0 + e * WG + (int)threadIdx.x, n - 1);
            s[e] = X[i];
            if (seed) {
                t[e] = C[2 * i + 1];
                k0[e] = key[i];
            }
        }
#pragma unroll
        for (int e = 0; e < kPer; ++e) {
            const int i = i0 + e * WG + (int)threadIdx.x;
            if (i >= n) break;
            xform_pt(Tl, s[e].x, s[e].y, s[e].z, s[e].x, s[e].y, s[e].z);
            X[i] = s[e];
            if (seed) key[i] = make_key(l2_simple(s[e].x, s[e].y, s[e].z, t[e].x, t[e].y, t[e].z), (uint32_t)key_idx(k0[e]));
        }
    }
}

constexpr int kTailPer = 4;  // fused test: points per thread per pipelined group

// SUMS: the tail also folds the next pass A's Σs (pair_cache_test); wave 0 folds, waves 1.. test, in
// index order.
template <int WG, int kPer, bool SUMS = false>
__device__ __forceinline__ int tail_group0(int n) {  // first (last-to-first) group's start
    constexpr int WW = SUMS ? WG - 64 : WG;
    const int kStep = WW * kPer, ngrp = (n + kStep - 1) / kStep;
    return (!SUMS ? ngrp - 1 : 0) * kStep;
}
template <int WG, int kPer, bool SUMS = false>
__device__ __forceinline__ void tail_prefetch(const WorkArgs& w, int p, int n, TailFirst<kPer>& f) {
    constexpr int WW = SUMS ? WG - 64 : WG;
    if (SUMS && threadIdx.x < 64) return;  // (the fold wave)
    const int wt = SUMS ? (int)threadIdx.x - 64 : (int)threadIdx.x;
    const int64_t xs = (int64_t)p * w.x_stride;
    const int i0 = tail_group0<WG, kPer, SUMS>(n);
#pragma unroll
    for (int e = 0; e < kPer; ++e) {
        const int i = min(i0 + e * WW + wt, n - 1);
        f.v[e] = w.X[xs + i];
        f.t[e] = w.nn_t[xs + i];
        f.U[e] = w.nn_u[xs + i];
    }
}

// ---------------------------------------------------------------------------------------------
// fold_update_kernel (PCL numerics): one workgroup per active pair.  Bit-exact float restatement
// of TransformationEstimationSVD (use_umeyama, Scalar = float) and calculateMSE: every sum is the
// sequential fold the reference performs, in correspondence (= source index) order, one lane per
// chain, over LDS chunks that the filler waves stage from the correspondence arrays while the
// fold lanes consume the previous chunk (double buffer: a fold never waits for a gather).
//  pass A: wave 0 lanes 0..6: Σs, Σd (Eigen 3.3 rowwise().sum(): fold from the first element ==
//          fold from -0.0f; Huber: fold of w·x from +0) and Σw (== |C| unweighted);
//          wave 1 lane 0: Σd² in double (MSE) — only when an MSE criterion is live (KParams::
//          need_mse), else wave 1 fills too.  Fillers: waves 2, 3.
//  pass B: wave 0 lanes 0..8: sigma(a, b) = Σ d'_a s'_b (float, from +0) over the float-demeaned
//          points; the fillers (waves 1..3) form the products (a*b, Huber (w*a)*b) so every chain is
//          a plain sum — IEEE addition is commutative, so p + acc == a*b + acc bit for bit.
// Rejected correspondences contribute the fold's identity (-0.0f / +0), i.e. nothing.
constexpr int kFoldWG = 256;
constexpr int kFoldWaves = kFoldWG / 64;

constexpr int kFoldRow = kFoldChunkP + kFoldPad;

// the fused test's LDS miss records (24 B each) after the bitmap and its prefixes, in the fold buffers
constexpr int kFoldRecs = ((2 * 9 * kFoldRow * 4 - 2 * kNeedWords * 4) / 24) & ~15;
// ... and with the Σs staging rows (pair_cache_test<SUMS>) at the buffers' end
constexpr int kFoldRecsSums = ((2 * 9 * kFoldRow * 4 - 2 * kNeedWords * 4 - 2 * kSumBuf * 4) / 24) & ~15;
struct FoldShared {
    alignas(16) float buf[2][9][kFoldRow];
    float res[8];
    int32_t cnt[kFoldWaves];
    int32_t mcount;  // tail: the pair's miss list length so far
    SolveShared s;
};

// The correspondences an update folds: the NN kernels' records C ({s.xyz, w}, {d.xyz, d²} per point),
// or, with the cached-neighbour test (C == nullptr), X_i (the searched point: the transform is
// deferred) and its NN's coordinates NT[i], d² = l2_simple(X_i, t) — the very expression the NN
// computed its key with, so the same bits.
struct FoldIn {
    const float4* C;
    const float4* X;
    const float4* NT;
    int n;
    uint64_t* tk = nullptr;  // debug (phase ticks, pair 0, thread 0): pass B's sub-phase stamps
    // key mode (WorkArgs::fold_keys, pass A only; C, NT null): the NN of X_i is TG[key_idx(K[i])], and
    // pass A writes the record pair corr_kernel would have written to Cw (pass B then reads them)
    const NNKey* K = nullptr;
    const float4* TG = nullptr;
    float4* Cw = nullptr;
    // lazy source cloud (the pair is pending, C null): the previous tail's transform, which it did not
    // store — X_i is Tp * X[i] (the expression that tail would have stored) unless X[i].w carries
    // kLazyFlag (the search re-wrote the point since: it is the moved one already)
    const float* Tp = nullptr;
};
// X_i of a pending pair from its stored record (FoldIn::Tp).  The transform is loaded here, at its use
// by a filler (scalar loads): held from the pass's start it stayed live through the fold waves' register
// groups and spilled them.
__device__ __forceinline__ void pend_pt(const float* Tp, float4& r0) {
    float Tq[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) Tq[k] = uload(Tp + k);
    float qx, qy, qz;
    xform_pt(Tq, r0.x, r0.y, r0.z, qx, qy, qz);
    const bool newer = l_flagged(r0.w);  // (selects per component: one of the whole records takes their addresses)
    r0.x = newer ? r0.x : qx;
    r0.y = newer ? r0.y : qy;
    r0.z = newer ? r0.z : qz;
}

// A running exact sum of non-negative doubles that are widened floats: S in units of 2^E (E = the
// lowest set bit's exponent over the nonzero terms so far), saturated at 2^53 — the argument of
// finish_kernel: while S < 2^53 the sequential double loop over the same terms never rounds, so its
// result is S * 2^E.  Each lane keeps its own (S, E) over the terms it is handed (no cross-lane step
// per chunk: the per-chunk wave reductions had cost as much as the float chains beside them);
// wave_exact_total combines the lanes (a lane's saturation means the whole total reaches 2^53).
constexpr uint64_t kExactSat = 1ull << 53;
__device__ __forceinline__ uint64_t exact_rescale(uint64_t S, int sh) {  // S * 2^sh, saturated (sh >= 0)
    return S == 0 ? 0 : ((sh >= 53 || (S >> (53 - sh)) != 0) ? kExactSat : (S << sh));
}
__device__ __forceinline__ void lane_exact_add(double x, uint64_t& S, int& E) {
    if (!(x > 0.0)) return;
    const uint64_t b = (uint64_t)__double_as_longlong(x);
    const int ex = (int)((b >> 52) & 0x7ff);
    const uint64_t mant = (b & ((1ull << 52) - 1)) | (1ull << 52);
    const int lo = ex - 1075 + (int)__builtin_ctzll(mant);
    if (lo < E) {  // re-express S in the finer unit (exact while it stays below 2^53)
        S = E == INT_MAX ? 0 : exact_rescale(S, E - lo);
        E = lo;
    }
    // x / 2^E = mant >> (E + 1075 - ex), a shift by at most ctz(mant): exact; below 2^53 iff ex - 1023 - E <= 52
    S = min(S + ((ex - 1023 - E <= 52) ? (mant >> (E + 1075 - ex)) : kExactSat), kExactSat);
}
__device__ __forceinline__ void wave_exact_total(uint64_t& S, int& E) {  // every lane ends with the wave's
    int e = E;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) e = min(e, __shfl_xor(e, off, 64));
    uint64_t t = E == INT_MAX ? 0 : exact_rescale(S, E - e);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) t = min(t + __shfl_xor(t, off, 64), kExactSat);
    S = t;
    E = e;
}

constexpr int kSliceGroup = 14;  // panels folded together (9 x 14 = 126 chains: two fold waves)
constexpr int kFillBatch = 2;  // a filler's correspondences in flight per round

// Pass A of the PCL-numerics update by a workgroup of WG threads over LDS chunks of CH points
// (buf: two chunks of 9 rows of ROW floats): wave 0 lanes 0..6 fold Σs, Σd (Eigen 3.3
// rowwise().sum(): from the first element == from -0.0f; Huber: w·x from +0) and Σw; wave 1 lane 0
// the double MSE chain when an MSE criterion is live (else it fills); the other waves stage the next
// chunk.  Leaves |C|, 1/n and the centroids in s.
// sums (fold_update_kernel, eligible pairs: every correspondence kept, unweighted, no MSE criterion):
// Σs as the previous update's tail folded it over the X it wrote — the fillers read nn_t only, and
// lanes 0..2 do not fold.
template <int WG, int CH, int ROW>
__device__ __forceinline__ void fold_pass_a(const KParams& kp, const FoldIn& f, float (*buf)[9][ROW], float* res,
                                            int32_t* wcnt, SolveShared& s, const float* sums = nullptr) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const bool weighted = kp.huber_delta < INFINITY;
    auto rec = [&](int i, float4& r0, float4& r1) {
        if (f.C) {
            r0 = f.C[2 * i];
            r1 = f.C[2 * i + 1];
        } else {
            r0 = f.X[i];
            r1 = f.NT[i];
        }
    };
    auto rec_fix = [&](float4& r0, float4& r1) {
        if (!f.C) {
            if (f.Tp) pend_pt(f.Tp, r0);
            const float d2 = l2_simple(r0.x, r0.y, r0.z, r1.x, r1.y, r1.z);
            r0.w = weighted ? (float)huber_w(d2, kp.huber_delta) : 1.0f;
            r1.w = d2;
        }
    };
    const int n = f.n;
    const int nch = (n + CH - 1) / CH;
    const bool mse = kp.need_mse != 0;  // wave 1 runs the MSE chain in pass A, else it fills
    const float ident = weighted ? 0.0f : -0.0f;
    const int fill0 = mse ? 128 : 64;  // first filler thread of pass A
    int cnt = 0;
    // Fillers issue every load of their (at most kPerA) elements before the first LDS store, so a
    // chunk costs one global round trip, not one per element.
    constexpr int kPerA = (CH + (WG - 128) - 1) / (WG - 128);
    // fill: load_a issues the loads of chunk c's records (clamped: at most kPerA per filler),
    // store_a turns them into the chain rows of LDS buffer c & 1.  (Loading two chunks ahead in two
    // register sets, here and in pass B, was measured slower: C3 update 176 -> 189 us per launch at two
    // pair groups — the batched update is bound by its bytes, not by these loads' latency.)
    auto load_a = [&](int c, float4 (&r)[kPerA][2]) __attribute__((always_inline)) {
        const int base = c * CH, len = min(CH, n - base), nf = WG - fill0;
        if (f.K) {  // key mode: X and the keys in flight together, then the targets they name
            uint32_t ti[kPerA];
#pragma unroll
            for (int e = 0; e < kPerA; ++e) {
                const int i = base + min(tid - fill0 + e * nf, len - 1);
                r[e][0] = f.X[i];
                ti[e] = (uint32_t)key_idx(f.K[i]);
            }
#pragma unroll
            for (int e = 0; e < kPerA; ++e) r[e][1] = f.TG[ti[e]];
            return;
        }
#pragma unroll
        for (int e = 0; e < kPerA; ++e) {
            const int i = base + min(tid - fill0 + e * nf, len - 1);
            if (sums)  // nn_t only (X's centroid is known)
                r[e][1] = f.NT[i];
            else
                rec(i, r[e][0], r[e][1]);
        }
    };
    auto store_a = [&](int c, float4 (&r)[kPerA][2]) __attribute__((always_inline)) {  // waves 2, 3 (and 1 without the MSE chain)
        float(*b)[ROW] = buf[c & 1];
        const int base = c * CH, len = min(CH, n - base), nf = WG - fill0;
#pragma unroll
        for (int e = 0; e < kPerA; ++e) {
            const int o = tid - fill0 + e * nf;
            if (o >= len) break;
            if (sums) {  // every correspondence kept, unweighted: Σd and Σw rows only
#pragma unroll
                for (int k = 0; k < 3; ++k) b[3 + k][o] = (&r[e][1].x)[k];
                b[6][o] = 1.0f;
                ++cnt;
                continue;
            }
            rec_fix(r[e][0], r[e][1]);
            const float d2 = r[e][1].w;
            if (f.Cw) {  // corr_kernel's record pair: {s.xyz, w}, {d.xyz, d²}
                f.Cw[2 * (base + o)] = r[e][0];
                f.Cw[2 * (base + o) + 1] = r[e][1];
            }
            const float sv[6] = {r[e][0].x, r[e][0].y, r[e][0].z, r[e][1].x, r[e][1].y, r[e][1].z};
            float v[6], wt = 0.0f, dd = 0.0f;
#pragma unroll
            for (int k = 0; k < 6; ++k) v[k] = ident;
            if (!(d2 > kp.max_d2)) {
                wt = r[e][0].w;
#pragma unroll
                for (int k = 0; k < 6; ++k) v[k] = weighted ? wt * sv[k] : sv[k];
                dd = d2;
                ++cnt;
            }
#pragma unroll
            for (int k = 0; k < 6; ++k) b[k][o] = v[k];
            b[6][o] = wt;
            reinterpret_cast<double*>(b[7])[o] = (double)dd;  // (rows 7-8: the MSE chain's doubles)
        }
    };
    float acc = (lane < 6) ? ident : 0.0f;
    double dacc = 0.0;
    // The roles run as separate wave-uniform loops (the same number of barriers in each), so the
    // fold lanes' register groups and the fillers' in-flight records are never live together.
    const int wv = __builtin_amdgcn_readfirstlane(wave);
    if (wv == 0) {
        const int lane0 = sums ? 3 : 0;
        fold_prio(true);
        for (int c = 0; c < nch; ++c) {
            __syncthreads();
            if (lane >= lane0 && lane < 7) acc = fold_seq<float>(buf[c & 1][lane], min(CH, n - c * CH), acc);
        }
        fold_prio(false);
    } else if (wv * 64 < fill0) {  // the MSE sum: its exact form, the whole wave per chunk
        uint64_t xs = 0;
        int xe = INT_MAX;
        for (int c = 0; c < nch; ++c) {
            __syncthreads();
            const double* dv = reinterpret_cast<const double*>(buf[c & 1][7]);
            const int len = min(CH, n - c * CH);
            for (int o = lane; o < len; o += 64) lane_exact_add(dv[o], xs, xe);
        }
        wave_exact_total(xs, xe);
        // -1: the span test failed (the sequential chain runs below)
        dacc = xs >= kExactSat ? -1.0 : (xe == INT_MAX ? 0.0 : ldexp((double)xs, xe));
    } else {
        if (nch > 0) {
            float4 r[kPerA][2];
            load_a(0, r);
            store_a(0, r);
        }
        for (int c = 0; c < nch; ++c) {
            __syncthreads();
            if (c + 1 < nch) {
                float4 r[kPerA][2];
                load_a(c + 1, r);
                store_a(c + 1, r);
            }
        }
    }
    // |C|: exact integer reduction of the fillers' counts
    cnt = wave_sumi(cnt);
    if (lane == 0) wcnt[wave] = cnt;
    if (wave == 0 && lane < 7) res[lane] = (sums && lane < 3) ? sums[lane] : acc;
    if (wave == 1 && lane == 0) s.mse_sum = dacc;  // 0 without the MSE chain (not used then)
    __syncthreads();
    if (tid == 0) {
        int total = 0;
        for (int k = 0; k < (WG / 64); ++k) total += wcnt[k];
        s.mom[0] = (double)total;
        // unweighted: one_over_n = 1/(float)n (fold of 1.0f == n exactly); Huber: 1/Σw
        const float one_over_n = 1.0f / res[6];
        s.one_over_n = one_over_n;
        for (int k = 0; k < 6; ++k) s.mean[k] = res[k] * one_over_n;
    }
    __syncthreads();
    if (mse && s.mse_sum < 0.0) {  // (uniform) the MSE terms span more than 53 bits: PCL's sequential
        dacc = 0.0;                 // double chain, over the chunks staged again (wave 0 idles)
        if (wv == 0) {
            for (int c = 0; c < nch; ++c) __syncthreads();
        } else if (wv * 64 < fill0) {
            for (int c = 0; c < nch; ++c) {
                __syncthreads();
                if (lane == 0) dacc = fold_seq_d(reinterpret_cast<const double*>(buf[c & 1][7]), min(CH, n - c * CH), dacc);
            }
        } else {
            if (nch > 0) {
                float4 r[kPerA][2];
                load_a(0, r);
                store_a(0, r);
            }
            for (int c = 0; c < nch; ++c) {
                __syncthreads();
                if (c + 1 < nch) {
                    float4 r[kPerA][2];
                    load_a(c + 1, r);
                    store_a(c + 1, r);
                }
            }
        }
        __syncthreads();  // (the last chunk folded before s.mse_sum is rewritten)
        if (wave == 1 && lane == 0) s.mse_sum = dacc;
        __syncthreads();
    }
}

// Pass B: sigma = one_over_n * Σ d'_a·s'_b over the float-demeaned correspondences, in Eigen 3.3's
// GEMM order (icp4r_math.hpp sigma_kc; oracle/icp_oracle.c umeyama_f32): the |C| correspondences are
// cut into S panels of kc, each panel's 9 coefficients are sequential float chains from +0, and the
// panels are added into sigma (from +0) as one_over_n * chain, in panel order.  The fillers form the
// products (Huber: (w·d'_a)·s'_b) and the fold lanes sum them (IEEE addition is commutative:
// p + acc == a·b + acc bit for bit).  Rejected correspondences (d² > max_d2) are not in PCL's list:
// they add the chain's identity (+0) where they fall, and panel boundaries are counted in accepted
// correspondences only (fold_bounds).
//  * one panel (|C| <= 680 at the default host facts): wave 0 lanes 0..8 fold the 9 chains over
//    chunks of CH points, as before;
//  * S panels: up to kSliceGroup panels at once — 9·G chains, one fold lane each (waves 0..1), over
//    LDS chunks that hold T steps of every panel of the group (row (panel, ab) of T floats, rows
//    strided ≡ 4 mod 8 floats so the fold lanes' ds_read_b128 hit distinct banks): the chain per
//    panel is kc long instead of |C|.
// Leaves the finished sigma in s.sigmaf.

// Panel starts of panels [s0, s0 + G] (point indices) when some correspondences are rejected: the
// panel of rank r starts at the point holding the (s·kc)-th accepted correspondence.  A scan over
// the points from the group's first start, WG at a time (ranks by ballot + wave prefix), until the
// group's last boundary is found.  bnd[0] must hold the group's first start; bnd[G] = n when s0 + G
// reaches S.
template <int WG, typename Acc>
__device__ __forceinline__ void fold_bounds(int n, int kc, int S, int s0, int G, Acc accepted, int32_t* bnd,
                                            int32_t* wsum) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    constexpr int NW = WG / 64;
    const int last = min(s0 + G, S);  // boundaries s0 + 1 .. last
    if (tid == 0 && last == S) bnd[last - s0] = n;
    int base = bnd[0];
    int running = s0 * kc;  // the rank of the first accepted correspondence at or after bnd[0]
    const int stop_rank = (last == S) ? INT_MAX : last * kc;
    while (base < n && running <= stop_rank) {
        const int i = base + tid;
        const bool acc = i < n && accepted(i);
        const uint64_t bal = __ballot(acc);
        const int pre = __builtin_popcountll(bal & ((1ull << lane) - 1ull));
        if (lane == 0) wsum[wave] = __builtin_popcountll(bal);
        __syncthreads();
        int off = running, tot = running;
#pragma unroll
        for (int v = 0; v < NW; ++v) {
            off += v < wave ? wsum[v] : 0;
            tot += wsum[v];
        }
        const int r = off + pre;
        if (acc && r > s0 * kc && r % kc == 0) {
            const int sl = r / kc;
            if (sl <= last && sl < S) bnd[sl - s0] = i;
        }
        running = tot;
        base += WG;
        __syncthreads();  // (wsum reused)
    }
    __syncthreads();
}

template <int WG, int CH, int ROW, bool PAR>
__device__ __forceinline__ void fold_pass_b(const KParams& kp, const FoldIn& f, float (*buf)[9][ROW], SolveShared& s) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const bool weighted = kp.huber_delta < INFINITY;
    auto rec = [&](int i, float4& r0, float4& r1) {
        if (f.C) {
            r0 = f.C[2 * i];
            r1 = f.C[2 * i + 1];
        } else {
            r0 = f.X[i];
            r1 = f.NT[i];
        }
    };
    auto rec_fix = [&](float4& r0, float4& r1) {
        if (!f.C) {
            if (f.Tp) pend_pt(f.Tp, r0);
            const float d2 = l2_simple(r0.x, r0.y, r0.z, r1.x, r1.y, r1.z);
            r0.w = weighted ? (float)huber_w(d2, kp.huber_delta) : 1.0f;
            r1.w = d2;
        }
    };
    const int n = f.n;
    if (f.tk) f.tk[19] = __builtin_amdgcn_s_memrealtime();
    const int wv = __builtin_amdgcn_readfirstlane(wave);
    const float ms[3] = {s.mean[0], s.mean[1], s.mean[2]};
    const float md[3] = {s.mean[3], s.mean[4], s.mean[5]};
    const float oon = s.one_over_n;
    const int cnt = (int)s.mom[0];
    const int kc = sigma_kc(cnt, kp.sigma_max_kc);
    const int S = (cnt > 0 && kc > 0) ? (cnt + kc - 1) / kc : 1;
    // the 9 products of one correspondence (0 when it is rejected)
    auto products = [&](float4 r0, float4 r1, float (&pr)[9]) __attribute__((always_inline)) {
        rec_fix(r0, r1);
        float sv[3] = {0.f, 0.f, 0.f}, dv[3] = {0.f, 0.f, 0.f}, wt = 0.f;
        if (!(r1.w > kp.max_d2)) {
            sv[0] = r0.x - ms[0];
            sv[1] = r0.y - ms[1];
            sv[2] = r0.z - ms[2];
            dv[0] = r1.x - md[0];
            dv[1] = r1.y - md[1];
            dv[2] = r1.z - md[2];
            wt = r0.w;
        }
#pragma unroll
        for (int ra = 0; ra < 3; ++ra)
#pragma unroll
            for (int rb = 0; rb < 3; ++rb) pr[ra * 3 + rb] = weighted ? (wt * dv[ra]) * sv[rb] : dv[ra] * sv[rb];
    };
    // every correspondence kept and unweighted (PCL's defaults): the products need no distance
    const bool plain = !weighted && cnt >= n;  // (nothing rejected in this iteration)
    auto products_plain = [&](float4 r0, const float4& r1, float (&pr)[9]) __attribute__((always_inline)) {
        if (f.Tp) pend_pt(f.Tp, r0);
        const float sv[3] = {r0.x - ms[0], r0.y - ms[1], r0.z - ms[2]};
        const float dv[3] = {r1.x - md[0], r1.y - md[1], r1.z - md[2]};
#pragma unroll
        for (int ra = 0; ra < 3; ++ra)
#pragma unroll
            for (int rb = 0; rb < 3; ++rb) pr[ra * 3 + rb] = dv[ra] * sv[rb];
    };
    if (!PAR || S <= 1) {
        // SEQ: wave 0 lanes 0..8 fold the 9 chains over the points of panels [0, npe) of the range
        // (panel k: [pb(k), pb(k + 1))) in point order, in chunks of up to CB; at each panel end
        // sigma += one_over_n * chain and the chain restarts from +0 — Eigen's panel order with one
        // lane per coefficient, the chain as long as the old single chain.  Chunks are not cut at
        // panel ends (a chunk's staging costs a round trip).  A panel end inside a chunk: the fillers
        // pad the ending panel's rows with +0 up to the next multiple of 32 and shift the new panel's
        // products behind it, so one fold_seq_switch rotation runs the row in whole groups (a
        // remainder would wait out an LDS round trip per few elements); such a chunk holds up to
        // CB - pad points.  Two panel ends in one chunk (only when kc < CB) take the unpadded slow
        // path (fold_span).  The chunk sequence is computed identically by the fold lanes and the
        // fillers (uniform arithmetic), so both run the same number of barriers.
        constexpr int CB = ROW - kFoldPad;  // row capacity (points + pad)
        constexpr int kFillB = WG - 64, kPerB = (CB + kFillB - 1) / kFillB;
        float sig = 0.0f, sacc = 0.0f;  // lane a*3+b of wave 0: sigma(a, b) and the open panel's chain
        struct Chunk {
            int c0, len, xs, k, nb;  // start, points, inner panel end (relative; INT_MAX: none), cursor
            bool multi;
        };
        auto seq = [&](auto pb, int npe) __attribute__((always_inline)) {
            const int p0 = pb(0), p1 = pb(npe);
            // chunk at c0 with the cursor (k, nb: the next panel end > c0)
            auto make = [&](int c0, int k, int nb) -> Chunk {
                Chunk ch;
                ch.c0 = c0;
                ch.k = k;
                ch.nb = nb;
                ch.len = min(CB, p1 - c0);
                ch.xs = INT_MAX;
                ch.multi = false;
                if (nb < c0 + ch.len) {
                    const int xs = nb - c0, xa = (xs + 31) & ~31;
                    ch.multi = k + 1 <= npe && pb(k + 1) < c0 + ch.len;
                    if (!ch.multi) {
                        if (xa >= CB) {
                            ch.len = xs;  // no room for the pad: the chunk ends with the panel
                        } else {
                            ch.xs = xs;
                            ch.len = min(ch.len, CB - (xa - xs));
                        }
                    }
                }
                return ch;
            };
            auto next = [&](const Chunk& ch) -> Chunk {  // the chunk after ch (past its panel ends)
                const int c1 = ch.c0 + ch.len;
                int k = ch.k, nb = ch.nb;
                while (nb <= c1) {
                    ++k;
                    nb = k <= npe ? pb(k) : INT_MAX;
                }
                return make(c1, k, nb);
            };
            auto load_b = [&](const Chunk& ch, float4 (&r)[kPerB][2]) __attribute__((always_inline)) {
#pragma unroll
                for (int e = 0; e < kPerB; ++e) {
                    const int i = ch.c0 + min(tid - 64 + e * kFillB, ch.len - 1);
                    rec(i, r[e][0], r[e][1]);
                }
            };
            auto store_b = [&](int c, const Chunk& ch, float4 (&r)[kPerB][2]) __attribute__((always_inline)) {
                float(*b)[ROW] = buf[c & 1];
                const int xs = ch.multi ? INT_MAX : ch.xs;
                const int padx = xs != INT_MAX ? ((xs + 31) & ~31) - xs : 0;
                if (plain) {
#pragma unroll
                    for (int e = 0; e < kPerB; ++e) {
                        const int o = tid - 64 + e * kFillB;
                        if (o >= ch.len) break;
                        float pr[9];
                        products_plain(r[e][0], r[e][1], pr);
                        const int at = o < xs ? o : o + padx;
#pragma unroll
                        for (int k = 0; k < 9; ++k) b[k][at] = pr[k];
                    }
                } else {
#pragma unroll
                    for (int e = 0; e < kPerB; ++e) {
                        const int o = tid - 64 + e * kFillB;
                        if (o >= ch.len) break;
                        float pr[9];
                        products(r[e][0], r[e][1], pr);
                        const int at = o < xs ? o : o + padx;
#pragma unroll
                        for (int k = 0; k < 9; ++k) b[k][at] = pr[k];
                    }
                }
                if (tid - 64 < padx)
#pragma unroll
                    for (int k = 0; k < 9; ++k) b[k][xs + tid - 64] = 0.0f;
            };
            Chunk ch = make(p0, 1, npe >= 1 ? pb(1) : INT_MAX);
            if (wv == 0) {
                int k = 1, nb = ch.nb;  // the next panel end
                fold_prio(true);
                for (int c = 0; ch.c0 < p1; ++c) {
                    __syncthreads();
                    const int c0 = ch.c0, c1 = c0 + ch.len;
                    const float* row = buf[c & 1][lane < 9 ? lane : 0];
                    if (!ch.multi) {
                        if (ch.xs == INT_MAX) {
                            if (lane < 9) sacc = fold_seq<float>(row, ch.len, sacc);
                        } else {
                            const int xa = (ch.xs + 31) & ~31;
                            if (lane < 9) {
                                // [0, xs) and the +0 pad into the ending chain, the rest into a new one
                                float acc2 = 0.0f;
                                fold_seq_switch<float>(row, xa + (ch.len - ch.xs), xa, sacc, acc2);
                                sig = sig + oon * sacc;  // res(i, j) += alpha * C0 into the zeroed sigma
                                sacc = acc2;
                            }
                            ++k;
                            nb = k <= npe ? pb(k) : INT_MAX;
                        }
                        if (nb == c1) {  // a panel ends with the chunk
                            if (lane < 9) sig = sig + oon * sacc;
                            sacc = 0.0f;
                            ++k;
                            nb = k <= npe ? pb(k) : INT_MAX;
                        }
                    } else {
                        int q = c0;
                        while (nb <= c1) {
                            if (lane < 9) {
                                sacc = fold_span<float>(row, q - c0, nb - c0, sacc);
                                sig = sig + oon * sacc;
                            }
                            sacc = 0.0f;
                            q = nb;
                            ++k;
                            nb = k <= npe ? pb(k) : INT_MAX;
                        }
                        if (q < c1 && lane < 9) sacc = fold_span<float>(row, q - c0, c1 - c0, sacc);
                    }
                    ch = next(ch);
                }
                fold_prio(false);
            } else {
                if (ch.c0 < p1) {
                    float4 r[kPerB][2];
                    load_b(ch, r);
                    store_b(0, ch, r);
                }
                for (int c = 0; ch.c0 < p1; ++c) {
                    __syncthreads();
                    ch = next(ch);  // the chunk to stage: c + 1
                    if (ch.c0 < p1) {
                        float4 r[kPerB][2];
                        load_b(ch, r);
                        store_b(c + 1, ch, r);
                    }
                }
            }
            __syncthreads();  // (the buffers are reused by the next range)
        };
        // the panels kSliceGroup at a time: their starts in s.bnd — (s0 + k) kc when every
        // correspondence is kept, else counted in accepted correspondences (fold_bounds)
        const bool rejected = cnt < n && S > 1;
        if (tid == 0) s.bnd[0] = 0;
        __syncthreads();
        for (int s0 = 0; s0 < S; s0 += kSliceGroup) {
            const int G = min(kSliceGroup, S - s0);
            if (rejected) {
                auto accepted = [&](int i) {
                    float4 r0, r1;
                    rec(i, r0, r1);
                    rec_fix(r0, r1);
                    return !(r1.w > kp.max_d2);
                };
                fold_bounds<WG>(n, kc, S, s0, G, accepted, s.bnd, s.wsum);
            } else {
                if (tid >= 1 && tid <= G) s.bnd[tid] = (s0 + tid >= S) ? n : (s0 + tid) * kc;
                __syncthreads();
            }
            seq([&](int k) { return s.bnd[k]; }, G);
            if (tid == 0) s.bnd[0] = s.bnd[G];
            __syncthreads();
        }
        if (wave == 0 && lane < 9) s.sigmaf[lane] = sig;
        __syncthreads();
        return;
    }

    // S panels, in groups of up to kSliceGroup
    constexpr int CAP = 9 * ROW;  // floats per chunk buffer
    auto bufs = [&](int k) -> float* { return &buf[k & 1][0][0]; };  // (no local array: it went to scratch)
    const bool rejected = cnt < n;  // some correspondence left PCL's list: panel starts by rank
    float sig = 0.0f;               // wave 0 lanes 0..8: sigma(a, b), the panels added in order
    if (tid == 0) s.bnd[0] = 0;
    __syncthreads();
    if (f.tk) f.tk[18] = __builtin_amdgcn_s_memrealtime();
    for (int s0 = 0; s0 < S; s0 += kSliceGroup) {
        const int G = min(kSliceGroup, S - s0);
        const int R = 9 * G;                                      // fold chains of the group
        const int FW = (R + 63) / 64;                             // fold waves (1 or 2)
        const int nF = WG - 64 * FW;                              // fillers
        if (rejected) {
            auto accepted = [&](int i) {
                float4 r0, r1;
                rec(i, r0, r1);
                rec_fix(r0, r1);
                return !(r1.w > kp.max_d2);
            };
            fold_bounds<WG>(n, kc, S, s0, G, accepted, s.bnd, s.wsum);
        }
        // panel sl of the group covers points [start(sl), start(sl + 1))
        auto start = [&](int sl) -> int {
            return rejected ? s.bnd[sl] : min((s0 + sl) * kc, n);
        };
        int maxlen = 0;
        for (int sl = 0; sl < G; ++sl) maxlen = max(maxlen, (s0 + sl + 1 >= S ? n : start(sl + 1)) - start(sl));
        // chunks of T steps per panel row, double-buffered (one chunk over both buffers, for the
        // 2k clouds' 4 panels, measured slower: its staging takes two round trips and hides nothing)
        const int stride = (((CAP / R) - 4) & ~7) + 4;           // row stride, ≡ 4 mod 8 floats
        const int T = stride - 4;                                 // steps per chunk (a multiple of 8)
        const float invT = 1.0f / (float)T;
        const int nch = (maxlen + T - 1) / T;
        // the fillers' slots of chunk c: slot q = (panel sl, step t), q = sl * T + t
        const int per = (G * T + nF - 1) / nF;
        auto fill = [&](int c) __attribute__((always_inline)) {
            float* b = bufs(c);
            const int me = tid - 64 * FW;
            for (int e0 = 0; e0 < per; e0 += kFillBatch) {
                float4 r[kFillBatch][2];
                int at[kFillBatch];
#pragma unroll
                for (int e = 0; e < kFillBatch; ++e) {
                    const int q = me + (e0 + e) * nF;
                    // q / T by a float reciprocal, corrected (exact for these small q)
                    int sl = (int)((float)q * invT), t = q - sl * T;
                    if (t >= T) { ++sl; t -= T; }
                    if (t < 0) { --sl; t += T; }
                    const int i0 = sl < G ? start(sl) : n;
                    const int i1 = sl < G ? (s0 + sl + 1 >= S ? n : start(sl + 1)) : n;
                    const int i = i0 + c * T + t;
                    at[e] = (e0 + e < per && sl < G && i < i1) ? sl * 9 * stride + t : -1;
                    rec(at[e] >= 0 ? i : 0, r[e][0], r[e][1]);
                }
#pragma unroll
                for (int e = 0; e < kFillBatch; ++e) {
                    if (at[e] < 0) continue;
                    float pr[9];
                    products(r[e][0], r[e][1], pr);
#pragma unroll
                    for (int k = 0; k < 9; ++k) b[at[e] + k * stride] = pr[k];
                }
            }
        };
        float acc = 0.0f;  // fold lane L = sl * 9 + ab: the chain of panel s0 + sl, coefficient ab
        const int L = tid;
        const int my_sl = L / 9;
        const int my_len = (wv < FW && L < R) ? ((s0 + my_sl + 1 >= S ? n : start(my_sl + 1)) - start(my_sl)) : 0;
        if (f.tk && s0 == 0) f.tk[0] = __builtin_amdgcn_s_memrealtime();
        if (wv >= FW && nch > 0) fill(0);
        for (int c = 0; c < nch; ++c) {
            __syncthreads();
            if (f.tk && s0 == 0 && c < 2) f.tk[c == 0 ? 1 : 16] = __builtin_amdgcn_s_memrealtime();
            if (wv < FW) {
                const int len = min(T, my_len - c * T);
                if (L < R && len > 0) acc = fold_row(bufs(c) + L * stride, len, acc);
                if (f.tk && s0 == 0 && c < 2) f.tk[15 + 2 * c] = __builtin_amdgcn_s_memrealtime();
            } else if (c + 1 < nch) {
                fill(c + 1);
            }
        }
        __syncthreads();  // every chunk folded: the buffer of chunk nch (unused) takes the chains
        if (f.tk && s0 == 0) f.tk[2] = __builtin_amdgcn_s_memrealtime();
        float* cs = bufs(nch);
        if (wv < FW && L < R) cs[L] = acc;
        __syncthreads();
        if (wave == 0 && lane < 9)
            for (int sl = 0; sl < G; ++sl) sig = sig + oon * cs[sl * 9 + lane];  // res += alpha * C0
        if (rejected && tid == 0) s.bnd[0] = s.bnd[G];  // the next group's first start
        __syncthreads();
    }
    if (wave == 0 && lane < 9) s.sigmaf[lane] = sig;
    __syncthreads();
    if (f.tk) f.tk[3] = __builtin_amdgcn_s_memrealtime();
}

// A pending pair (WorkArgs::lazy_x) that no storing tail follows — it converged or failed in this update, or
// no further iteration runs: the store its silent tail left out, made now.  An unflagged point becomes
// Tp * X with the bounds moved (that tail's expressions), a flagged one only loses its flag, so the
// pair's stored state is the one every tail storing would have left.
template <int WG>
__device__ __forceinline__ void flush_pending(const WorkArgs& w, int p, int n, const float* Tp) {
    float Tq[16];
#pragma unroll
    for (int q = 0; q < 16; ++q) Tq[q] = uload(Tp + q);
    const int64_t xs = (int64_t)p * w.x_stride;
    float4* X = w.X + xs;
    float* uu = w.nn_u + xs;
    constexpr int kPer = 4;  // (every load of a round before its first store, as transform_pair)
    for (int i0 = 0; i0 < n; i0 += WG * kPer) {
        float4 v[kPer];
        float U[kPer];
#pragma unroll
        for (int e = 0; e < kPer; ++e) {
            const int i = min(i0 + e * WG + (int)threadIdx.x, n - 1);
            v[e] = X[i];
            U[e] = uu[i];
        }
#pragma unroll
        for (int e = 0; e < kPer; ++e) {
            const int i = i0 + e * WG + (int)threadIdx.x;
            if (i >= n) break;
            float4 q = v[e];
            xform_pt(Tq, v[e].x, v[e].y, v[e].z, q.x, q.y, q.z);
            const float2 Lq = move_lu(make_float2(v[e].w, U[e]), v[e].x, v[e].y, v[e].z, q.x, q.y, q.z);
            q.w = Lq.x;
            if (l_flagged(v[e].w)) {
                v[e].w = fabsf(v[e].w);
                X[i] = v[e];
            } else {
                X[i] = q;
                uu[i] = Lq.y;
            }
        }
    }
}

// The update of pair p; returns the pair's work in the next pass (its misses in the fused test; 0
// when it is not searched again).
// silent (launch-uniform, WorkArgs::lazy_x): this launch's fused tail stores neither X nor U — unless the
// pair is pending already (never two silent tails in a row: one flag bit tells two states apart, not three).
// PEND (WorkArgs::lazy_x): the launch follows a silent tail, so its active pairs are pending — whether
// a pass is pending is launch-uniform (the host loop's parity), and as a template argument the other
// launches compile to the code they had (the pending forms cost registers: scalar ones for T_pend).
template <bool PEND>
__device__ __forceinline__ int fold_update_pair(const PairArgs& a, const WorkArgs& w, int tail_test, int silent, int p,
                                                FoldShared& sh) {
    PairState& st = w.state[p];
    if (st.phase != kPhaseActive) return 0;
    const int tid = threadIdx.x;
    const int n = a.src_n[p];
    clear_need(w, p, n, tid, kFoldWG);
    const int64_t xs = w.x_stride;
    const KParams& kp = a.kp;
    const float4* C = w.corr ? w.corr + (int64_t)p * xs * 2 : nullptr;
    const float4* Xp = w.X + (int64_t)p * xs;
    const float4* NT = w.nn_t ? w.nn_t + (int64_t)p * xs : nullptr;

    const bool ticks = w.ticks != nullptr && p == 0 && tid == 0;
    if (ticks) w.ticks[0] = __builtin_amdgcn_s_memrealtime();
#if ICP4R_WG_TICKS  // diagnostic build: every pair's phase stamps in its 10th update (tools/experiments/wg_ticks.py)
    uint64_t* wt = (w.ticks && tid == 0 && st.iterations == 9) ? w.ticks + 32 + 4 * (int64_t)gridDim.x + 8 * (int64_t)p
                                                              : nullptr;
    if (wt) {
        wt[0] = __builtin_amdgcn_s_memrealtime();
        // where the fold wave (wave 0) runs: HW_ID (SIMD [5:4], CU [11:8], SH [12], SE [15:13]) and XCC_ID
        wt[5] = (uint64_t)(uint32_t)__builtin_amdgcn_s_getreg(4 | (31 << 11)) |
                ((uint64_t)(uint32_t)__builtin_amdgcn_s_getreg(20 | (31 << 11)) << 32);
    }
#define WG_TICK(k) \
    if (wt) wt[k] = __builtin_amdgcn_s_memrealtime()
#else
#define WG_TICK(k)
#endif
    // lazy source cloud: the previous tail was silent — passes A and B form T_pend * X themselves
    const bool lazy = w.lazy_x && w.nn_u && !C && !w.sums_tail;  // (launch-uniform)
    // (PEND: every active pair of the launch is pending — the tails alternate, and a pair that stops is flushed)
    const float* Tp = PEND ? st.T_pend : nullptr;
    FoldIn fin{C, Xp, NT, n};
    fin.Tp = Tp;
    // the previous tail folded this pass A's Σs (w.sums_tail: eligible registrations; the flag is the
    // pair's, set only by a tail that ran)
    const bool sums_tail = w.sums_tail && tail_test && w.nn_u && !C;  // (launch-uniform)
    const bool use_sums = sums_tail && uload(&st.sums_ok) == 1;
    fold_pass_a<kFoldWG, kFoldChunkP, kFoldRow>(kp, fin, sh.buf, sh.res, sh.cnt, sh.s, use_sums ? st.sum_s : nullptr);
    if (use_sums && tid == 0) st.sums_ok = 0;
    if (ticks) w.ticks[1] = __builtin_amdgcn_s_memrealtime();
    WG_TICK(1);
    fold_pass_b<kFoldWG, kFoldChunkP, kFoldRow, false>(kp, fin, sh.buf, sh.s);
    if (ticks) w.ticks[2] = __builtin_amdgcn_s_memrealtime();
    WG_TICK(2);
    // the fused test's first point group is loaded, and its LDS bitmap cleared, while thread 0 solves
    const bool tail = tail_test && w.nn_u;
    int nwork = 0;
    TailFirst<kTailPer> tf;
    uint32_t* need = reinterpret_cast<uint32_t*>(&sh.buf[0][0][0]);  // the fold buffers are free now
    if (tail) {
        // (the Σs-folding tail loads its first group itself: a second prefetch layout held across the
        // solve spilled to scratch)
        // (n = 0: no group to load — its first group would start a whole group before the pair's slots)
        if (!sums_tail && n > 0) tail_prefetch<kFoldWG, kTailPer>(w, p, n, tf);
        for (int k = tid; k < ((n + 31) >> 5); k += kFoldWG) need[k] = 0u;
        if (tid == 0) sh.mcount = 0;
    }
    if (tid == 0) solve_pair<kNumericsPCL>(sh.s, st, kp);
    __syncthreads();
    if (ticks) w.ticks[3] = __builtin_amdgcn_s_memrealtime();
    WG_TICK(3);
    if (Tp && !(tail && sh.s.flag == 0)) {  // no tail follows to make the pending store
        flush_pending<kFoldWG>(w, p, n, Tp);
        if (tid == 0) st.pending = 0;
    }
    if (sh.s.flag == 1) return 0;  // error: PCL breaks before transforming
    if (!w.defer_xform) transform_pair<kFoldWG>(w, p, n, sh.s.T_inc, w.seed_next && w.corr);
    // The next pass's cached-neighbour test, fused (tail_test: another iteration follows and the pair
    // is still active): the same work as nn_cache_test_kernel for this pair — the deferred
    // transformCloud(T_inc), the bounds moved, the test, hit keys, the miss bitmap — done here, where
    // its HBM stream overlaps the other workgroups' latency-bound fold chains instead of taking a
    // launch of its own.  The workgroup owns the pair, so the bitmap is built in LDS and stored whole.
    if (tail && sh.s.flag == 0) {
        // the fold buffers: the bitmap (cleared above), its word prefixes and the LDS miss records
        int32_t* pre = reinterpret_cast<int32_t*>(need + kNeedWords);
        float4* lv = reinterpret_cast<float4*>(pre + kNeedWords);
        uint2* lm = reinterpret_cast<uint2*>(lv + (sums_tail ? kFoldRecsSums : kFoldRecs));
        float T[16];
#pragma unroll
        for (int q = 0; q < 16; ++q) T[q] = sh.s.T_inc[q];
#if ICP4R_WG_TICKS
        uint64_t* stamp = wt ? wt + 6 : nullptr;
#else
        uint64_t* stamp = nullptr;
#endif
        if (sums_tail) {
            // the staging rows of the Σs fold at the end of the fold buffers, the miss records before
            float* stg = reinterpret_cast<float*>(&sh.buf[0][0][0]) + (2 * 9 * kFoldRow - 2 * kSumBuf);
            nwork = pair_cache_test<kFoldWG, kSumPer, false, true>(
                a, w, p, n, T, need, pre, lv, lm, kFoldRecsSums, &sh.mcount, sh.cnt, false, stamp, nullptr, stg,
                st.sum_s, &st.sums_ok);
        } else {
            const bool quiet = lazy && silent && !Tp;
            nwork = pair_cache_test<kFoldWG, kTailPer, false>(a, w, p, n, T, need, pre, lv, lm, kFoldRecs,
                                                                    &sh.mcount, sh.cnt, false, stamp, &tf, nullptr,
                                                                    nullptr, nullptr, Tp, quiet);
            if (quiet) {  // the transform this tail tested at and did not store
                if (tid < 16) st.T_pend[tid] = sh.s.T_inc[tid];
                if (tid == 0) st.pending = 1;
            } else if (Tp && tid == 0) {
                st.pending = 0;
            }
        }
    }
    if (ticks) w.ticks[4] = __builtin_amdgcn_s_memrealtime();
    WG_TICK(4);
    return nwork;
}

// order_ncu > 0: the next pass's work list is built here, by the launch's last workgroup (the
// nn_order_kernel launch and its kernel boundary removed from every iteration pass).  Every
// workgroup publishes its pair's work word (an agent-scope store: write-through, past every cache),
// waits for it, then counts itself in with an agent-scope add; the workgroup whose add completes
// the launch's count reads the words back with agent-scope (L1-bypassing) loads.  The counter only
// grows (plist_n[3], zeroed per registration): a launch's last add is the one that makes it a
// multiple of the grid size.
// Ordering: this is the measured-valid hand-off of MI355X_MICROARCH.md §Workgroup dispatch (the
// first row of its sc1 table): ONE lane per workgroup, its payload (owork[p]) stored sc1
// (write-through) and drained with s_waitcnt vmcnt(0) before the agent-scope add; the consumer is the
// workgroup whose add came last, told by the add's return value, and every load of the payload is an
// sc1 load issued after that add returned (the other waves: after the barrier below).  The asm
// statement's "memory" clobber keeps the compiler from moving the store past the add.  An acq_rel add
// would instead put an L2 write-back (buffer_wbl2) in every workgroup — 1.7-6.5 us each by the same
// section's price list — for an ordering the sc1 accesses already give.
// (launch bound: 4 workgroups per CU; 3 and 2, held down with dynamic LDS, were the experiment)
template <bool PEND>
__global__ __launch_bounds__(kFoldWG, 4) void fold_update_kernel(PairArgs a, WorkArgs w, int tail_test, int order_ncu,
                                                                             int silent) {
    __shared__ FoldShared sh;
    __shared__ OrderShared osh;
    __shared__ int32_t last;
    const int p = xcd_remap(blockIdx.x, gridDim.x);
    const int nwork = fold_update_pair<PEND>(a, w, tail_test, silent, p, sh);
    if (order_ncu <= 0) return;
    if (threadIdx.x == 0) {
        __hip_atomic_store(w.owork + p, nwork, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const int old = __hip_atomic_fetch_add(w.plist_n + 3, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        last = (old + 1) % (int)gridDim.x == 0 ? 1 : 0;
    }
    __syncthreads();
    if (!last) return;
    order_items<kFoldWG, true>(a, w, (int)gridDim.x, 0, 0, order_ncu, osh);
}

// ---------------------------------------------------------------------------------------------
// fold_update_res_kernel (round 6): the batched update with the pair's points read from HBM once and
// held on chip across pass A, pass B and the fused test.  fold_update_kernel streams X and nn_t three
// times per launch (pass A, pass B, the tail: 1.01 GB for 268 MB of clouds at C3); here a 256-thread
// workgroup holds its pair's <= 8192 points — thread t, column j: point t + 256 j — two workgroups per
// CU: X_i.xyz and the NN's x, y in registers (160 VGPRs), the NN's z and L_i = X_i.w in LDS (L rounded
// down to half precision: a lower bound stays a lower bound, so the cached-neighbour test stays exact —
// a miss is searched — and every result is unchanged).
//  loads:  8 columns' X and nn_t in flight at a time, one batch ahead of pass A's folds;
//  pass A: two columns at a time staged from registers into LDS rows, wave 0 lanes 0..6 fold the seven
//          sequential float chains (Σs, Σd, Σw) over them; |C| is a reduction, and the MSE sum (when a
//          criterion is live) its exact integer form per thread (fold_update_kernel's argument), with
//          PCL's sequential double chain over re-read points as the fallback;
//  pass B: Eigen's panels side by side (fold_pass_b<PAR>'s arithmetic): every thread writes the
//          products of its points whose step (index mod kc) falls into the chunk into the panel rows,
//          117 fold lanes sum them (a correspondence rejected for an overflowing d²: fold_pass_b over
//          re-read points);
//  tail:   the next pass's cached-neighbour test from the held points, U read once; a miss's tag
//          (nn_t.w: positions) read for the misses only.
// Per point and iteration: X and nn_t read (32 B), U read (4 B), X and U written (20 B) — the
// one-read bytes.  Results are bit-identical to fold_update_kernel (the parity tests run both).
constexpr int kResWG = 256;
constexpr int kResCols = kResMaxN / kResWG;  // points per thread: column j = points [256 j, 256 j + 256)
constexpr int kResRowA = kResWG + kFoldPad;  // pass A: one column per chunk
constexpr int kResStage = 7680;              // staging floats (30 KB): pass A rows, pass B panel rows, the
                                             // fallbacks' buffers, the tail's bitmap, prefixes and records
constexpr int kResRecs = ((kResStage - 2 * kNeedWords) * 4 / 24) & ~15;  // the tail's LDS miss records
static_assert(kResMaxN == kResWG * kResCols && kResCols % 8 == 0 && kResCols <= 32, "columns");
static_assert(2 * 7 * kResRowA <= kResStage, "pass A rows");
struct ResShared {
    float qz[kResMaxN];     // the NN's z
    _Float16 L[kResMaxN];   // X_i.w rounded down: the test's lower bounds
    alignas(16) float stage[kResStage];
    float res[8];
    int32_t cnt[kResWG / 64];
    uint64_t mse_s[kResWG / 64];
    int32_t mse_e[kResWG / 64];
    int32_t mcount;
    SolveShared s;
};

typedef float fcols __attribute__((ext_vector_type(kResCols)));  // one coordinate of a thread's columns
typedef uint32_t ucols __attribute__((ext_vector_type(kResCols)));
__device__ __forceinline__ int uni(int j) { return __builtin_amdgcn_readfirstlane(j); }

// x rounded toward -inf to half precision (a lower bound stays one)
__device__ __forceinline__ _Float16 half_down(float x) {
    _Float16 h = (_Float16)x;
    if ((float)h > x) {
        uint16_t b = __builtin_bit_cast(uint16_t, h);
        b = (b & 0x8000u) ? (uint16_t)(b + 1) : (b == 0 ? (uint16_t)0x8001u : (uint16_t)(b - 1));
        h = __builtin_bit_cast(_Float16, b);
    }
    return h;
}

__device__ __forceinline__ int res_update_pair(const PairArgs& a, const WorkArgs& w, int tail_test, int p,
                                               ResShared& sh) {
    PairState& st = w.state[p];
    if (st.phase != kPhaseActive) return 0;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = a.src_n[p];  // <= kResMaxN (launch_update)
    clear_need(w, p, n, tid, kResWG);
    const int64_t xs = (int64_t)p * w.x_stride;
    const float4* Xp = w.X + xs;
    const float4* NT = w.nn_t + xs;
    const KParams& kp = a.kp;
    const bool mse = kp.need_mse != 0;
    const int ncol = (n + kResWG - 1) / kResWG;
    float* const buf = sh.stage;
#if ICP4R_WG_TICKS  // diagnostic build: every pair's phase stamps in its 10th update (tools/experiments/wg_ticks.py)
    uint64_t* wt = (w.ticks && tid == 0 && st.iterations == 9) ? w.ticks + 32 + 4 * (int64_t)gridDim.x + 8 * (int64_t)p
                                                              : nullptr;
#define RES_TICK(k) \
    if (wt) wt[k] = __builtin_amdgcn_s_memrealtime()
    // pair 0's finer stamps (pass A per column, pass B per chunk) after every pair's 8 slots
    uint64_t* wx = (wt && p == 0) ? w.ticks + 32 + 12 * (int64_t)gridDim.x : nullptr;
#define RES_TICKX(k) \
    if (wx) wx[k] = __builtin_amdgcn_s_memrealtime()
#else
#define RES_TICK(k)
#define RES_TICKX(k)
#endif
    RES_TICK(0);

    // ---- the pair, read once, in batches of 8 columns one batch ahead of pass A's folds.  The columns
    // are register vectors indexed by a wave-uniform column number (s_set_gpr_idx: one instruction per
    // access), so every loop over them is a loop, not 32 unrolled copies — an unrolled kernel's code
    // (~0.5 MB) had been fetched from L2 instruction by instruction
    fcols px, py, pz, qx, qy;
    constexpr int kLB = 4;  // columns' loads in flight at a time
    float4 lv_[kLB], lt_[kLB];  // a batch in flight
    auto issue = [&](int b) __attribute__((always_inline)) {
#pragma unroll
        for (int e = 0; e < kLB; ++e) {
            const int j = uni(b * kLB + e), i = min(tid + kResWG * j, n - 1);
            if (j < ncol) {
                lv_[e] = Xp[i];
                lt_[e] = NT[i];
            }
        }
    };
    auto extract = [&](int b) __attribute__((always_inline)) {
#pragma unroll
        for (int e = 0; e < kLB; ++e) {
            const int j = uni(b * kLB + e), i = tid + kResWG * j;
            if (j < ncol) {
                px[j] = lv_[e].x;
                py[j] = lv_[e].y;
                pz[j] = lv_[e].z;
                qx[j] = lt_[e].x;
                qy[j] = lt_[e].y;
                sh.qz[i] = lt_[e].z;  // (past n: point n - 1's, never read)
                sh.L[i] = half_down(lv_[e].w);
            }
        }
    };
    issue(0);
    extract(0);
    if (ncol > kLB) issue(1);
    RES_TICK(7);

    // ---- pass A: chunk K = columns 2K, 2K + 1 staged into buffer K & 1 (rows Σs.xyz, Σd.xyz, Σw)
    int cnt = 0;
    uint32_t amask = 0;  // bit j: point t + 256 j is a correspondence (d² <= max_d2)
    uint64_t ms_s = 0;
    int ms_e = INT_MAX;
    auto stage_col = [&](int j) __attribute__((always_inline)) {
        j = uni(j);
        const int i = tid + kResWG * j;
        if (i >= n) return;
        float* b = buf + (j & 1) * 7 * kResRowA + tid;
        const float z = sh.qz[i];
        const float d2 = l2_simple(px[j], py[j], pz[j], qx[j], qy[j], z);
        const bool ok = !(d2 > kp.max_d2);  // (max_d2 = FLT_MAX: only an overflowing d² is rejected)
        b[0] = ok ? px[j] : -0.0f;
        b[kResRowA] = ok ? py[j] : -0.0f;
        b[2 * kResRowA] = ok ? pz[j] : -0.0f;
        b[3 * kResRowA] = ok ? qx[j] : -0.0f;
        b[4 * kResRowA] = ok ? qy[j] : -0.0f;
        b[5 * kResRowA] = ok ? z : -0.0f;
        b[6 * kResRowA] = ok ? 1.0f : 0.0f;
        cnt += ok ? 1 : 0;
        amask |= ok ? 1u << j : 0u;
        if (mse) lane_exact_add(ok ? (double)d2 : 0.0, ms_s, ms_e);
    };
    float acc = (lane < 6) ? -0.0f : 0.0f;  // Eigen's rowwise().sum() from the first element; Σw from 0
    if (ncol > 0) stage_col(0);
    for (int K = 0; K < ncol; ++K) {
        __syncthreads();  // column K staged; buffer (K + 1) & 1 folded (column K - 1)
        if (wave == 0 && lane < 7) {
            fold_prio(true);
            acc = fold_row(buf + ((K & 1) * 7 + lane) * kResRowA, min(kResWG, n - K * kResWG), acc);
            fold_prio(false);
        }
        RES_TICKX(K);
        // the next batch of columns arrives before column K + 1 needs it; the one after goes in flight
        if ((K + 1) % kLB == 0 && K + 1 < ncol) {
            extract((K + 1) / kLB);
            if (K + 1 + kLB < ncol) issue((K + 1) / kLB + 1);
        }
        if (K + 1 < ncol) stage_col(K + 1);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) cnt += __shfl_xor(cnt, off, 64);
    if (mse) wave_exact_total(ms_s, ms_e);
    if (lane == 0) {
        sh.cnt[wave] = cnt;
        sh.mse_s[wave] = ms_s;
        sh.mse_e[wave] = ms_e;
    }
    if (wave == 0 && lane < 7) sh.res[lane] = acc;
    __syncthreads();
    if (tid == 0) {
        int total = 0;
        for (int k = 0; k < kResWG / 64; ++k) total += sh.cnt[k];
        sh.s.mom[0] = (double)total;
        // unweighted: one_over_n = 1/(float)n (fold of 1.0f == n exactly)
        const float one_over_n = 1.0f / sh.res[6];
        sh.s.one_over_n = one_over_n;
        for (int k = 0; k < 6; ++k) sh.s.mean[k] = sh.res[k] * one_over_n;
        double msum = 0.0;  // (0 without an MSE criterion: not used then)
        if (mse) {  // the waves' exact sums combined (-1: the terms span more than 53 bits)
            int e = INT_MAX;
            for (int k = 0; k < kResWG / 64; ++k) e = min(e, sh.mse_e[k]);
            uint64_t t = 0;
            for (int k = 0; k < kResWG / 64; ++k)
                t = min(t + (sh.mse_e[k] == INT_MAX ? 0 : exact_rescale(sh.mse_s[k], sh.mse_e[k] - e)), kExactSat);
            msum = t >= kExactSat ? -1.0 : (e == INT_MAX ? 0.0 : ldexp((double)t, e));
        }
        sh.s.mse_sum = msum;
    }
    __syncthreads();
    if (mse && sh.s.mse_sum < 0.0) {
        // (rare) the terms span more than 53 bits: PCL's sequential double chain (calculateMSE) over the
        // points' d² (rejected: +0, which changes no partial sum), re-read from HBM a column at a time so
        // that no register of the held pair is needed; thread 0 adds them in order
        double* db = reinterpret_cast<double*>(buf);
        double dacc = 0.0;
        for (int c = 0; c < ncol; ++c) {
            const int i = c * kResWG + tid;
            if (i < n) {
                const float4 v = Xp[i], t = NT[i];
                const float d2 = l2_simple(v.x, v.y, v.z, t.x, t.y, t.z);
                db[tid] = (double)(!(d2 > kp.max_d2) ? d2 : 0.0f);
            }
            __syncthreads();
            if (tid == 0)
                for (int k = 0, len = min(kResWG, n - c * kResWG); k < len; ++k) dacc = dacc + db[k];
            __syncthreads();
        }
        if (tid == 0) sh.s.mse_sum = dacc;
        __syncthreads();
    }
    RES_TICK(1);

    // ---- pass B: sigma in Eigen's panel order, the panels side by side (fold_pass_b<PAR>'s arithmetic).
    // A point's step is its rank among the correspondences (its index when every point is one) mod kc.
    {
        const int cntA = (int)sh.s.mom[0];
        const bool plain = cntA >= n;
        int32_t* base = reinterpret_cast<int32_t*>(buf);  // (rejections: rank of (column, wave)'s first point)
        if (!plain) {
            for (int j = 0; j < ncol; ++j) {
                const uint64_t bal = __ballot((amask >> j) & 1u);
                if (lane == 0) base[j * 4 + wave] = __builtin_popcountll(bal);
            }
            __syncthreads();
            if (wave == 0) {  // exclusive scan in point order (column-major, then wave)
                const int c0 = lane < 2 * ncol ? base[2 * lane] : 0, c1 = lane < 2 * ncol ? base[2 * lane + 1] : 0;
                int incl = c0 + c1;
#pragma unroll
                for (int off = 1; off < 64; off <<= 1) {
                    const int o = __shfl_up(incl, off, 64);
                    if (lane >= off) incl += o;
                }
                if (lane < 2 * ncol) {
                    base[2 * lane] = incl - c0 - c1;
                    base[2 * lane + 1] = incl - c1;
                }
            }
            __syncthreads();
        }
        // rank of point t + 256 j among the correspondences (-1: rejected); every lane calls it
        auto rank = [&](int j) __attribute__((always_inline)) -> int {
            if (plain) return tid + kResWG * j < n ? tid + kResWG * j : -1;
            const uint32_t on = (amask >> j) & 1u;
            const uint64_t bal = __ballot(on);
            const int r = base[j * 4 + wave] +
                          (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(bal >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bal, 0u));
            return on ? r : -1;
        };
        const float oon = sh.s.one_over_n;
        const int kc = sigma_kc(cntA, kp.sigma_max_kc);
        const int S = (cntA > 0 && kc > 0) ? (cntA + kc - 1) / kc : 1;
        const float invkc = 1.0f / (float)kc;
        float sig = 0.0f;  // wave 0 lanes 0..8: sigma(a, b), the panels added in order
        for (int s0 = 0; s0 < S; s0 += kSliceGroup) {
            const int G = min(kSliceGroup, S - s0);
            const int R = 9 * G;                                   // fold chains of the group
            const int stride = (((kResStage / R) - 4) & ~7) + 4;  // one buffer: rows of T steps, ≡ 4 mod 8
            const int T = stride - 4;
            const int r0 = s0 * kc;                                // the group's first rank
            const int r1 = min((s0 + G) * kc, cntA);
            const int nch = (min(kc, r1 - r0) + T - 1) / T;
            // fold lane L = sl * 9 + ab: the chain of panel s0 + sl, coefficient ab
            const int my_len = tid < R ? min(kc, cntA - (s0 + tid / 9) * kc) : 0;
            const float invT = 1.0f / (float)T;
            // (rejections) each column's point in this group: chunk | panel << 8 | step in the chunk << 16
            // (chunk 255: none) — one register per column, read by the chunk scan with the column index
            ucols info;
            if (!plain) {
#pragma unroll
            for (int j = 0; j < kResCols; ++j) {
                uint32_t v = 255u;
                if (j < ncol) {
                    const int r = rank(j) - r0;
                    if (r >= 0 && r < r1 - r0) {
                        int sl = (int)((float)r * invkc);  // r / kc, corrected (exact for these r)
                        int sp = r - sl * kc;
                        if (sp >= kc) { ++sl; sp -= kc; }
                        if (sp < 0) { --sl; sp += kc; }
                        int c = (int)((float)sp * invT);
                        if (c * T > sp) --c;
                        if ((c + 1) * T <= sp) ++c;
                        v = (uint32_t)min(c, 254) | ((uint32_t)sl << 8) | ((uint32_t)(sp - c * T) << 16);
                    }
                }
                info[j] = v;
            }
            }
            if (s0 == 0) RES_TICK(5);
            float accp = 0.0f;
            for (int c = 0; c < nch; ++c) {
                const int w0 = c * T;  // the chunk's first step
                // the means, re-read per chunk as wave-uniform (SGPR) values: hoisted out of the chunk
                // loop, the demeaned coordinates had gone to scratch
                float mv[6];
#pragma unroll
                for (int k = 0; k < 6; ++k) {
                    mv[k] = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(sh.s.mean[k])));
                    asm volatile("" : "+s"(mv[k]));
                }
                const float ms0 = mv[0], ms1 = mv[1], ms2 = mv[2], md0 = mv[3], md1 = mv[4], md2 = mv[5];
                // every thread writes the products of its points whose step lies in [w0, w0 + T)
                auto put = [&](int j, uint32_t sl, uint32_t tt) __attribute__((always_inline)) {
                    const int i = tid + kResWG * j;
                    const float sv0 = px[j] - ms0, sv1 = py[j] - ms1, sv2 = pz[j] - ms2;
                    const float dv0 = qx[j] - md0, dv1 = qy[j] - md1, dv2 = sh.qz[i] - md2;
                    float* o = buf + sl * 9 * stride + tt;
                    o[0] = dv0 * sv0;
                    o[stride] = dv0 * sv1;
                    o[2 * stride] = dv0 * sv2;
                    o[3 * stride] = dv1 * sv0;
                    o[4 * stride] = dv1 * sv1;
                    o[5 * stride] = dv1 * sv2;
                    o[6 * stride] = dv2 * sv0;
                    o[7 * stride] = dv2 * sv1;
                    o[8 * stride] = dv2 * sv2;
                };
                if (plain) {
                    // a point's rank is its index: panel sl's steps [w0, w0 + T) are the points [a, b), in
                    // one or two columns (wave-uniform bounds)
                    for (int sl = 0; sl < G; ++sl) {
                        const int a = r0 + sl * kc + w0;
                        const int b = min(a + T, min(r0 + (sl + 1) * kc, r1));
                        for (int j0 = a / kResWG; a < b && j0 <= (b - 1) / kResWG; ++j0) {
                            const int j = uni(j0);
                            const int i = tid + kResWG * j;
                            if (i >= a && i < b) put(j, (uint32_t)sl, (uint32_t)(i - a));
                        }
                    }
                } else {
                    for (int j0 = 0; j0 < ncol; ++j0) {
                        const int j = uni(j0);
                        const uint32_t v = info[j];
                        if ((v & 255u) == (uint32_t)c) put(j, (v >> 8) & 255u, v >> 16);
                    }
                }
                __syncthreads();  // the chunk staged
                if (s0 == 0) RES_TICKX(32 + 2 * c);
                if (tid < R) {
                    const int len = min(T, my_len - w0);
                    if (len > 0) accp = fold_row(buf + tid * stride, len, accp);
                }
                __syncthreads();  // the chunk folded: the buffer is free
                if (s0 == 0) RES_TICKX(33 + 2 * c);
            }
            if (tid < R) buf[tid] = accp;
            __syncthreads();
            if (wave == 0 && lane < 9)
                for (int k = 0; k < G; ++k) sig = sig + oon * buf[k * 9 + lane];  // res += alpha * C0
            __syncthreads();
        }
        if (wave == 0 && lane < 9) sh.s.sigmaf[lane] = sig;
    }
    RES_TICK(2);

    // ---- the solve (thread 0), the tail's bitmap cleared meanwhile
    uint32_t* need = reinterpret_cast<uint32_t*>(buf);  // (pass B's buffers are free)
    int32_t* pre = reinterpret_cast<int32_t*>(need + kNeedWords);
    float4* lv = reinterpret_cast<float4*>(pre + kNeedWords);
    uint2* lm = reinterpret_cast<uint2*>(lv + kResRecs);
    static_assert(2 * kNeedWords * 4 + kResRecs * 24 <= kResStage * 4, "tail records");
    // the tail's U, every column in flight across the solve (one register per column)
    const bool tail = tail_test && w.nn_u;
    float* uu = w.nn_u + xs;
    fcols uv;
    if (tail) {
#pragma unroll
        for (int j = 0; j < kResCols; ++j)
            if (j < ncol) uv[j] = uu[min(tid + kResWG * j, n - 1)];
        for (int k = tid; k < ((n + 31) >> 5); k += kResWG) need[k] = 0u;
        if (tid == 0) sh.mcount = 0;
    }
    __syncthreads();  // (sigmaf, and pass B's last reads of the buffer)
    if (tid == 0) solve_pair_body<kNumericsPCL>(sh.s, st, kp);
    __syncthreads();
    RES_TICK(3);
    if (sh.s.flag != 0 || !tail) return 0;  // error, converged, or no further pass

    // ---- tail: the next pass's cached-neighbour test (pair_cache_test's arithmetic)
    float T[16];  // (wave-uniform: SGPR operands of the transform)
#pragma unroll
    for (int q = 0; q < 16; ++q) T[q] = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(sh.s.T_inc[q])));
    float4* X = w.X + xs;
    float4* sqg = w.sq + xs;
    uint2* smg = w.sm + xs;
    int hits = 0, misses = 0;
    for (int j0 = 0; j0 < ncol; ++j0) {
        const int j = uni(j0);
        const int i = tid + kResWG * j;
        const bool valid = i < n;
        float ox, oy, oz;
        xform_pt(T, px[j], py[j], pz[j], ox, oy, oz);  // PCL transformCloud, in place
        const float2 Lm = move_lu(make_float2((float)sh.L[i], uv[j]), px[j], py[j], pz[j], ox, oy, oz);
        const float d2 = l2_simple(ox, oy, oz, qx[j], qy[j], sh.qz[i]);
        const bool hit = valid & cache_hit(Lm.x, d2);
        if (valid) {
            X[i] = make_float4(ox, oy, oz, Lm.x);
            uu[i] = Lm.y;
        }
        const bool miss = valid && !hit;
        const int k = wave_append(miss, &sh.mcount);
        if (hit) {
            ++hits;
        } else if (miss) {  // the record without its positions (nn_t.w: read below, for the misses only)
            if (k < kResRecs) {
                lv[k] = make_float4(ox, oy, oz, Lm.y);
                lm[k] = make_uint2((uint32_t)i, 0u);
            } else {
                sqg[k] = make_float4(ox, oy, oz, Lm.y);
                smg[k] = make_uint2((uint32_t)i, 0u);
            }
            ++misses;
        }
    }
    RES_TICK(6);
    // every record appended: the overflow records' stores drained before the barrier (another wave
    // reads them back below, with L1-bypassing loads)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    // the misses' positions: nn_t.w (the NN's sorted target position | the query's sorted position)
    const int tot = sh.mcount;
    for (int k0 = tid; k0 < tot; k0 += 4 * kResWG) {
        uint32_t ii[4];
        float tg[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int k = min(k0 + e * kResWG, tot - 1);
            ii[e] = k < kResRecs ? lm[k].x
                                 : __hip_atomic_load(reinterpret_cast<uint32_t*>(smg + k), __ATOMIC_RELAXED,
                                                     __HIP_MEMORY_SCOPE_AGENT);
            ii[e] = min(ii[e], (uint32_t)(n - 1));  // (a record's index is below n)
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) tg[e] = NT[ii[e]].w;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int k = k0 + e * kResWG;
            if (k >= tot) break;
            const uint32_t sp = nt_pos(tg[e]);
            atomicOr(&need[sp >> 5], 1u << (sp & 31));
            const uint2 m = make_uint2(ii[e] | (nt_tpos(tg[e]) << kNtPosShift), sp);
            if (k < kResRecs)
                lm[k] = m;
            else
                smg[k] = m;
        }
    }
    const int tp = test_place<kResWG>(w, p, n, hits, misses, need, pre, lv, lm, kResRecs, sh.cnt, false, nullptr);
    RES_TICK(4);
#undef RES_TICK
#undef RES_TICKX
    return tp;
}

__global__ __launch_bounds__(kResWG, 2) void fold_update_res_kernel(PairArgs a, WorkArgs w, int tail_test,
                                                                     int order_ncu) {
    __shared__ ResShared sh;
    __shared__ OrderShared osh;
    __shared__ int32_t last;
    const int p = xcd_remap(blockIdx.x, gridDim.x);
    const int nwork = res_update_pair(a, w, tail_test, p, sh);
    if (order_ncu <= 0) return;
    // the next pass's work list by the launch's last workgroup (fold_update_kernel's hand-off)
    if (threadIdx.x == 0) {
        __hip_atomic_store(w.owork + p, nwork, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const int old = __hip_atomic_fetch_add(w.plist_n + 3, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        last = (old + 1) % (int)gridDim.x == 0 ? 1 : 0;
    }
    __syncthreads();
    if (!last) return;
    order_items_body<kResWG, true>(a, w, (int)gridDim.x, 0, 0, order_ncu, osh);
}

// ---------------------------------------------------------------------------------------------
// fold_update_wide_kernel: the update of plans with at most one pair per CU (single pairs — the node's
// per-frame call, C1 / C2 / C5 — and small batches; no fused cache test, no fused work list): one
// 1024-thread workgroup and most of the CU's LDS per pair.  Pass A is the same sequential centroid
// chains over larger chunks; pass B runs the sigma panels side by side (fold_pass_b<PAR>: up to 14
// panels, 9 chains each, over chunks of 128 steps per panel), so its chain is one panel (kc) long
// instead of |C|, and the 14 filler waves stage a chunk in one round trip.  Same results bit for bit
// as fold_update_kernel (the parity tests run both; plan option wide_update = 0 selects the narrow one).
constexpr int kWideWG = 1024;
constexpr int kWideChunkP = 1792;  // points per pass-A chunk; pass B: 9 x 14 panel rows of 128 steps
constexpr int kWideRow = kWideChunkP + kFoldPad;
struct WideShared {
    alignas(16) float buf[2][9][kWideRow];
    float res[8];
    int32_t cnt[kWideWG / 64];
    int32_t lay[5];  // fold_update_held_kernel: pass B's layout (kc, S, stride, T, chunks), by thread 0
    SolveShared s;
};

__global__ __launch_bounds__(kWideWG) void fold_update_wide_kernel(PairArgs a, WorkArgs w) {
    __shared__ WideShared sh;
    const int p = xcd_remap(blockIdx.x, gridDim.x);
    PairState& st = w.state[p];
    if (st.phase != kPhaseActive) return;
    const int tid = threadIdx.x;
    const int n = a.src_n[p];
    clear_need(w, p, n, tid, kWideWG);
    const int64_t xs = w.x_stride;
    const KParams& kp = a.kp;
    const float4* C = w.corr ? w.corr + (int64_t)p * xs * 2 : nullptr;
    const float4* Xp = w.X + (int64_t)p * xs;
    const float4* NT = w.nn_t ? w.nn_t + (int64_t)p * xs : nullptr;
    const bool ticks = w.ticks != nullptr && p == 0 && tid == 0;
    if (ticks) w.ticks[0] = __builtin_amdgcn_s_memrealtime();
    const FoldIn fin{C, Xp, NT, n, ticks ? w.ticks + 12 : nullptr};
    // fold_keys: pass A reads X and the merged keys' targets and writes the records pass B reads
    // (corr_kernel's work, without its launch)
    FoldIn fa = fin;
    if (w.fold_keys && C) {
        fa.C = nullptr;
        fa.K = w.nn_key + (int64_t)p * xs;
        fa.TG = a.tgt + a.tgt_off[p];
        fa.Cw = const_cast<float4*>(C);
    }
    fold_pass_a<kWideWG, kWideChunkP, kWideRow>(kp, fa, sh.buf, sh.res, sh.cnt, sh.s);
    if (ticks) w.ticks[1] = __builtin_amdgcn_s_memrealtime();
    fold_pass_b<kWideWG, kWideChunkP, kWideRow, true>(kp, fin, sh.buf, sh.s);
    if (ticks) w.ticks[2] = __builtin_amdgcn_s_memrealtime();
    if (tid == 0) solve_pair<kNumericsPCL>(sh.s, st, kp);
    __syncthreads();
    if (ticks) w.ticks[3] = __builtin_amdgcn_s_memrealtime();
    if (sh.s.flag == 1) return;  // error: PCL breaks before transforming
    if (!w.defer_xform) transform_pair<kWideWG>(w, p, n, sh.s.T_inc, w.seed_next && w.corr);
    if (ticks) w.ticks[4] = __builtin_amdgcn_s_memrealtime();
}

// ---------------------------------------------------------------------------------------------
// fold_update_held_kernel<HOLD, S0> (round 6): fold_update_wide_kernel for sources of at most
// HOLD x F points (F filler threads: <3, true> up to 2,112 — the node's 2k C1 scan, F = 704; <10, false>
// up to 8,960 — the 8k scans of C2 / C5, F = 896), with the pair's correspondence records read from
// HBM once per update.  The filler threads (waves 2..15; S0: but 4, 8, 12) load their records (record
// i is filler i mod F's slot i / F) — chunk 0's two slots first, the rest after the first barrier —
// and keep each as six floats in registers (s and d; d² and the weight are
// recomputed — the search formed the record's d² as l2_simple(s, d) and its weight from that, with
// contraction off, so the same bits): pass A's chunk c is slots 2c and 2c + 1 of every filler (LDS
// stores only, no round trip per chunk), and pass B's panel chunks take each record's nine products
// from the filler that holds it — the wide kernel's fill of every pass-B chunk was a global round trip
// (C1: pass B 7.7 -> 5.2 us; 2.3 us of it had been the first fill).  Waves 0 and 1 (the fold lanes,
// the MSE wave) hold nothing: the roles run as separate wave-uniform loops, so the held records are
// never live beside fold_seq's 96 registers.  The chains, their orders and the panel adds are
// fold_pass_a / fold_pass_b<PAR>'s, so the results are the wide kernel's bit for bit; pass B takes that
// kernel's global path when a correspondence was rejected or weighted (the panels then start by rank),
// for one panel, or for more panels than one group.
constexpr int kHeldFill0 = 128;                       // first filler thread
// S0 (the small form): waves 4, 8 and 12 — the fold wave's SIMD partners (wave w runs on SIMD w mod 4)
// — hold and stage nothing, so that wave 0's add chains run alone on their SIMD: 11 filler waves
template <bool S0>
constexpr int held_fillers() { return S0 ? 11 * 64 : kWideWG - kHeldFill0; }  // 704 / 896
static_assert(2 * held_fillers<false>() <= kWideChunkP, "pass A's chunk fits the wide buffers");
// pass B's first chunk in the small form (steps; 0: every chunk T steps).  Measured (two A/B rounds):
// C1 0.384 (0) / 0.381 (128) / 0.385 (64) / 0.388 ms (32); at 8k any ramp lost (C2 1.162 -> 1.175
// with 128, 1.197 with 32), so the 8k form keeps uniform chunks.
constexpr int kHeldPassBRamp = 128;
static_assert(kHeldMaxN == 10 * held_fillers<false>() && kHeldSmallN == 3 * held_fillers<true>(), "held sizes");

// PCL's sequential double chain over LDS, few registers (the MSE fallback beside the held records)
__device__ __forceinline__ double fold_seq_d_lite(const double* f, int len, double acc) {
    int k = 0;
    for (; k + 8 <= len; k += 8) {
        const double2 g0 = *reinterpret_cast<const double2*>(f + k), g1 = *reinterpret_cast<const double2*>(f + k + 2);
        const double2 g2 = *reinterpret_cast<const double2*>(f + k + 4), g3 = *reinterpret_cast<const double2*>(f + k + 6);
        acc = acc + g0.x;
        acc = acc + g0.y;
        acc = acc + g1.x;
        acc = acc + g1.y;
        acc = acc + g2.x;
        acc = acc + g2.y;
        acc = acc + g3.x;
        acc = acc + g3.y;
    }
    for (; k < len; ++k) acc = acc + f[k];
    return acc;
}

template <int HOLD, bool S0>
__global__ __launch_bounds__(kWideWG) void fold_update_held_kernel(PairArgs a, WorkArgs w) {
    constexpr int kHeldFillers = held_fillers<S0>();
    constexpr int kPassBRamp = S0 ? kHeldPassBRamp : 0;
    constexpr int kHeldCH = 2 * kHeldFillers;  // pass A chunk: two slots of every filler
    __shared__ WideShared sh;
    const int p = xcd_remap(blockIdx.x, gridDim.x);
    if (w.ticks != nullptr && p == 0 && threadIdx.x == 0) w.ticks[9] = __builtin_amdgcn_s_memrealtime();
    PairState& st = w.state[p];
    if (st.phase != kPhaseActive) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wv = __builtin_amdgcn_readfirstlane(wave);
    const int n = a.src_n[p];
    const int64_t xs = w.x_stride;
    const KParams& kp = a.kp;
    const float4* C = w.corr ? w.corr + (int64_t)p * xs * 2 : nullptr;
    const float4* Xp = w.X + (int64_t)p * xs;
    const float4* NT = w.nn_t ? w.nn_t + (int64_t)p * xs : nullptr;
    const bool ticks = w.ticks != nullptr && p == 0 && tid == 0;
    // key mode (w.fold_keys): X and the merged keys' targets; the records are written for pass B's
    // global path (corr_kernel's work, as in the wide kernel)
    const bool keys = w.fold_keys && C;
    const NNKey* K = keys ? w.nn_key + (int64_t)p * xs : nullptr;
    const float4* TG = keys ? a.tgt + a.tgt_off[p] : nullptr;
    const bool weighted = kp.huber_delta < INFINITY;
    const bool mse = kp.need_mse != 0;
    const float ident = weighted ? 0.0f : -0.0f;
    const int nch = (n + kHeldCH - 1) / kHeldCH;
    // filler slot column: waves 2..15 (S0: but 4, 8, 12 — the idle waves, `idle`)
    const bool idle = S0 && wv >= 2 && (wv & 3) == 0;
    const int f = S0 ? (wv - 2 - (wv >> 2)) * 64 + lane : tid - kHeldFill0;

    // the records (fillers only: loaded inside pass A's filler branch, so that they are never live in
    // the fold wave's branch — a load ahead of the role branches had kept them live there)
    float sx[HOLD], sy[HOLD], sz[HOLD], dx[HOLD], dy[HOLD], dz[HOLD];
    // pass B's layout (fold_pass_b<PAR>: S panels of kc, rows of T steps strided stride) and each held
    // record's place in it, packed: offset << 4 | chunk + 1 (0: none)
    constexpr int CAP = 9 * kWideRow;
    auto layout = [&](int cnt_, int& kc, int& S, int& stride, int& T, int& nchb) __attribute__((always_inline)) {
        kc = sigma_kc(cnt_, kp.sigma_max_kc);
        S = (cnt_ > 0 && kc > 0) ? (cnt_ + kc - 1) / kc : 1;
        stride = (((CAP / max(9 * S, 18)) - 4) & ~7) + 4;
        T = stride - 4;
        // chunks of a ramp: kPassBRamp steps first, doubling up to T (the first chunk's fill is on the
        // critical path; the later fills overlap the folds before them).  More panels than one group
        // (rows too short, down to T = 0 for hundreds of panels) take pass B's global path: 15 chunks
        // stands for "not held" there, and no loop runs on such a layout.
        nchb = 15;
        if (S <= kSliceGroup && T >= 8) {
            nchb = 0;
            for (int b = 0, len = kPassBRamp > 0 ? min(T, kPassBRamp) : T; b < kc; b += len, len = min(T, 2 * len)) ++nchb;
        }
    };
    int pk[HOLD];
    auto held_offsets = [&](int cnt_) __attribute__((always_inline)) {
        int kc, S, stride, T, nchb;
        layout(cnt_, kc, S, stride, T, nchb);
        if (nchb > 14) return;  // (pass B's global path: no offsets needed, and no loop on T = 0)
        // (the panel by a float reciprocal, corrected: exact for these small operands; the chunk by
        // walking the ramp)
        const float invkc = 1.0f / (float)kc;
#pragma unroll
        for (int k = 0; k < HOLD; ++k) {
            const int i = f + k * kHeldFillers;
            int q = (int)((float)i * invkc);
            int t = i - q * kc;
            if (t >= kc) { ++q; t -= kc; }
            if (t < 0) { --q; t += kc; }
            int c = 0, len = kPassBRamp > 0 ? min(T, kPassBRamp) : T;
            while (t >= len) {
                t -= len;
                len = min(T, 2 * len);
                ++c;
            }
            pk[k] = i < n ? ((q * 9 * stride + t) << 4) | (c + 1) : 0;
        }
    };
    clear_need(w, p, n, tid, kWideWG);
    if (ticks) w.ticks[0] = __builtin_amdgcn_s_memrealtime();

    // ---- pass A (fold_pass_a's chains over chunks of kHeldCH points)
    int cnt = 0;
    // slots 2c, 2c + 1 of this filler -> chunk c (first staging, key mode: and corr_kernel's record pair
    // {s.xyz, w}, {d.xyz, d²} for pass B's global path — per chunk, so that chunk 0 waits for its own
    // slots' gathers only)
    auto store_a = [&](int c, bool first) __attribute__((always_inline)) {
        float(*b)[kWideRow] = sh.buf[c & 1];
#pragma unroll
        for (int k = 0; k < HOLD; ++k) {
            if ((k >> 1) != c) continue;
            const int i = k * kHeldFillers + f;
            if (i >= n) continue;
            const int o = i - c * kHeldCH;
            const float d2 = l2_simple(sx[k], sy[k], sz[k], dx[k], dy[k], dz[k]);
            const float sv[6] = {sx[k], sy[k], sz[k], dx[k], dy[k], dz[k]};
            if (keys && first) {
                const float w0 = weighted ? (float)huber_w(d2, kp.huber_delta) : 1.0f;
                w.corr[(int64_t)p * xs * 2 + 2 * i] = make_float4(sx[k], sy[k], sz[k], w0);
                w.corr[(int64_t)p * xs * 2 + 2 * i + 1] = make_float4(dx[k], dy[k], dz[k], d2);
            }
            float v[6], wt = 0.0f, dd = 0.0f;
#pragma unroll
            for (int q = 0; q < 6; ++q) v[q] = ident;
            if (!(d2 > kp.max_d2)) {
                wt = weighted ? (float)huber_w(d2, kp.huber_delta) : 1.0f;
#pragma unroll
                for (int q = 0; q < 6; ++q) v[q] = weighted ? wt * sv[q] : sv[q];
                dd = d2;
                ++cnt;
            }
#pragma unroll
            for (int q = 0; q < 6; ++q) b[q][o] = v[q];
            b[6][o] = wt;
            reinterpret_cast<double*>(b[7])[o] = (double)dd;
        }
    };
    float acc = (lane < 6) ? ident : 0.0f;
    double dacc = 0.0;
    if (wv == 0) {
        fold_prio(true);
        for (int c = 0; c < nch; ++c) {
            __syncthreads();
            if (ticks && c < 6) w.ticks[20 + c] = __builtin_amdgcn_s_memrealtime();
            if (lane < 7) acc = fold_seq<float>(sh.buf[c & 1][lane], min(kHeldCH, n - c * kHeldCH), acc);
        }
        fold_prio(false);
        if (ticks) w.ticks[26] = __builtin_amdgcn_s_memrealtime();
    } else if (wv == 1) {
        if (mse) {  // the MSE sum's exact form (fold_pass_a), the whole wave per chunk
            uint64_t xsum = 0;
            int xe = INT_MAX;
            for (int c = 0; c < nch; ++c) {
                __syncthreads();
                const double* dv = reinterpret_cast<const double*>(sh.buf[c & 1][7]);
                const int len = min(kHeldCH, n - c * kHeldCH);
                for (int o = lane; o < len; o += 64) lane_exact_add(dv[o], xsum, xe);
            }
            wave_exact_total(xsum, xe);
            dacc = xsum >= kExactSat ? -1.0 : (xe == INT_MAX ? 0.0 : ldexp((double)xsum, xe));
        } else {
            for (int c = 0; c < nch; ++c) __syncthreads();
        }
    } else if (idle) {
        for (int c = 0; c < nch; ++c) __syncthreads();
    } else {
        // the held records, every load in flight together (16-B loads: with the two modes' loads
        // merged, a pointer that lost its alignment was split into four dword loads — 2.4 us more)
        // (chunk 0's two slots first, staged, then the other slots' loads, which land during chunk 0's
        // fold: issued all together, every wave's later slots queued ahead of the other waves' first
        // ones and chunk 0 waited for nearly all of them — the fold started 3.6 us in at 8k)
        auto load = [&](int k0, int k1) __attribute__((always_inline)) {
            if (keys) {
                uint32_t ti[HOLD];
#pragma unroll
                for (int k = 0; k < HOLD; ++k) {
                    if (k < k0 || k >= k1) continue;
                    const int i = min(f + k * kHeldFillers, n - 1);
                    const float4 x = Xp[i];
                    sx[k] = x.x;
                    sy[k] = x.y;
                    sz[k] = x.z;
                    ti[k] = (uint32_t)key_idx(K[i]);
                }
#pragma unroll
                for (int k = 0; k < HOLD; ++k) {
                    if (k < k0 || k >= k1) continue;
                    const float4 t = TG[ti[k]];
                    dx[k] = t.x;
                    dy[k] = t.y;
                    dz[k] = t.z;
                }
            } else {
#pragma unroll
                for (int k = 0; k < HOLD; ++k) {
                    if (k < k0 || k >= k1) continue;
                    const int i = min(f + k * kHeldFillers, n - 1);
                    const float4* q0 = static_cast<const float4*>(__builtin_assume_aligned(C ? C + 2 * i : Xp + i, 16));
                    const float4* q1 = static_cast<const float4*>(__builtin_assume_aligned(C ? C + 2 * i + 1 : NT + i, 16));
                    const float4 r0 = *q0, r1 = *q1;
                    sx[k] = r0.x;
                    sy[k] = r0.y;
                    sz[k] = r0.z;
                    dx[k] = r1.x;
                    dy[k] = r1.y;
                    dz[k] = r1.z;
                }
            }
        };
        // (an empty source holds nothing: the clamped index n - 1 would be -1, in front of the pair's
        // slots, and in key mode no key of the pair has been written for the gather to follow)
        if (n > 0) load(0, 2);
        store_a(0, true);
        for (int c = 0; c < nch; ++c) {
            __syncthreads();
            if (c == 0) load(2, HOLD);  // (after the barrier: the fold of chunk 0 starts meanwhile)
            if (c + 1 < nch) store_a(c + 1, true);
        }
        // pass B's chunk offsets for the plain case (every correspondence kept: kc = sigma_kc(n)),
        // while the fold wave finishes (14 filler waves on 4 SIMDs: ~1.3 us of VALU at 8k if left to
        // pass B's critical path)
        held_offsets(n);
    }
    // |C|: exact integer reduction of the fillers' counts (DPP: wave 0 runs it after its chain)
    cnt = wave_sumi(cnt);
    if (lane == 0) sh.cnt[wave] = cnt;
    if (wave == 0 && lane < 7) sh.res[lane] = acc;
    if (wave == 1 && lane == 0) sh.s.mse_sum = dacc;
    __syncthreads();
    if (tid == 0) {
        int total = 0;
        for (int k = 0; k < kWideWG / 64; ++k) total += sh.cnt[k];
        sh.s.mom[0] = (double)total;
        const float one_over_n = 1.0f / sh.res[6];
        sh.s.one_over_n = one_over_n;
        for (int k = 0; k < 6; ++k) sh.s.mean[k] = sh.res[k] * one_over_n;
        // pass B's layout, once (its integer divisions in every lane of 16 waves had cost ~1 us of
        // VALU on pass B's critical path)
        layout(total, sh.lay[0], sh.lay[1], sh.lay[2], sh.lay[3], sh.lay[4]);
    }
    __syncthreads();
    if (mse && sh.s.mse_sum < 0.0) {  // (uniform) PCL's sequential double chain over the chunks again
        dacc = 0.0;
        if (wv == 0 || idle) {
            for (int c = 0; c < nch; ++c) __syncthreads();
        } else if (wv == 1) {
            for (int c = 0; c < nch; ++c) {
                __syncthreads();
                if (lane == 0)
                    dacc = fold_seq_d_lite(reinterpret_cast<const double*>(sh.buf[c & 1][7]), min(kHeldCH, n - c * kHeldCH),
                                           dacc);
            }
        } else {
            store_a(0, false);
            for (int c = 0; c < nch; ++c) {
                __syncthreads();
                if (c + 1 < nch) store_a(c + 1, false);
            }
        }
        __syncthreads();
        if (wave == 1 && lane == 0) sh.s.mse_sum = dacc;
        __syncthreads();
    }
    if (ticks) w.ticks[1] = __builtin_amdgcn_s_memrealtime();

    // ---- pass B
    SolveShared& s = sh.s;
    const int cntC = (int)s.mom[0];
    const int kc = sh.lay[0], S = sh.lay[1], stride = sh.lay[2], T = sh.lay[3], nchb = sh.lay[4];
    const int G = S, R = 9 * G, FW = (R + 63) / 64;
    if (weighted || cntC < n || S <= 1 || S > kSliceGroup || nchb > 14) {
        const FoldIn fin{C, Xp, NT, n};
        fold_pass_b<kWideWG, kWideChunkP, kWideRow, true>(kp, fin, sh.buf, s);
    } else {
        // every correspondence kept, unweighted: panel sl = [sl kc, min((sl + 1) kc, n)), one group of
        // S panels (fold_pass_b<PAR>'s layout: row (panel, ab) of T steps, rows strided = 4 mod 8)
        const float ms[3] = {s.mean[0], s.mean[1], s.mean[2]};
        const float md[3] = {s.mean[3], s.mean[4], s.mean[5]};
        const float oon = s.one_over_n;
        auto bufs = [&](int k) -> float* { return &sh.buf[k & 1][0][0]; };
        float sig = 0.0f, pacc = 0.0f;
        if (wv < 2) {
            const int L = tid;
            const int my_sl = L / 9;
            const int my_len = (wv < FW && L < R) ? min(kc, n - my_sl * kc) : 0;
            for (int c = 0, cb = 0, cl = kPassBRamp > 0 ? min(T, kPassBRamp) : T; c < nchb; ++c, cb += cl, cl = min(T, 2 * cl)) {
                __syncthreads();
                if (ticks && c < 2) w.ticks[28 + c] = __builtin_amdgcn_s_memrealtime();
                const int len = min(cl, my_len - cb);
                if (wv < FW && L < R && len > 0) pacc = fold_row(bufs(c) + L * stride, len, pacc);
            }
            if (ticks) w.ticks[30] = __builtin_amdgcn_s_memrealtime();
        } else if (idle) {
            for (int c = 0; c < nchb; ++c) __syncthreads();
        } else {
            // each held record's LDS offset in its chunk's buffer and the chunk (-1: none), by a
            // float reciprocal of kc, corrected
            // (pk: from pass A — cntC == n here, the layout it assumed)
            auto fill = [&](int c) __attribute__((always_inline)) {
                float* b = bufs(c);
#pragma unroll
                for (int k = 0; k < HOLD; ++k) {
                    if ((pk[k] & 15) != c + 1) continue;
                    const int off = pk[k] >> 4;
                    const float sv[3] = {sx[k] - ms[0], sy[k] - ms[1], sz[k] - ms[2]};
                    const float dv[3] = {dx[k] - md[0], dy[k] - md[1], dz[k] - md[2]};
                    float* o = b + off;
#pragma unroll
                    for (int ra = 0; ra < 3; ++ra)
#pragma unroll
                        for (int rb = 0; rb < 3; ++rb) o[(ra * 3 + rb) * stride] = dv[ra] * sv[rb];
                }
            };
            fill(0);
            if (w.ticks != nullptr && p == 0 && lane == 0) w.ticks[32 + wave - 2] = __builtin_amdgcn_s_memrealtime();
            for (int c = 0; c < nchb; ++c) {
                __syncthreads();
                if (c + 1 < nchb) fill(c + 1);
            }
        }
        __syncthreads();  // every chunk folded: the buffer of chunk nchb (unused) takes the chains
        float* cs = bufs(nchb);
        if (wv < FW && tid < R) cs[tid] = pacc;
        __syncthreads();
        if (wave == 0 && lane < 9)
            for (int sl = 0; sl < G; ++sl) sig = sig + oon * cs[sl * 9 + lane];  // res += alpha * C0
        if (wave == 0 && lane < 9) s.sigmaf[lane] = sig;
        __syncthreads();
    }
    if (ticks) w.ticks[2] = __builtin_amdgcn_s_memrealtime();
    if (tid == 0) solve_pair_body<kNumericsPCL>(sh.s, st, kp);  // (inline: no call's register saves)
    __syncthreads();
    if (ticks) w.ticks[3] = __builtin_amdgcn_s_memrealtime();
    if (sh.s.flag == 1) return;  // error: PCL breaks before transforming
    if (!w.defer_xform) transform_pair<kWideWG>(w, p, n, sh.s.T_inc, w.seed_next && w.corr);
    if (ticks) w.ticks[4] = __builtin_amdgcn_s_memrealtime();
}

// ---------------------------------------------------------------------------------------------
// update_kernel (F64 numerics): one workgroup per active pair: correspondences -> double moments
// (fixed-order block reduction) -> solve -> convergence -> X := T_inc * X.
constexpr int kUpdWG = 512;
constexpr int kUpdWaves = kUpdWG / 64;

__global__ __launch_bounds__(kUpdWG) void update_f64_kernel(PairArgs a, WorkArgs w) {
    constexpr int NM = MomLayout<kNumericsF64>::N;
    constexpr int I_CNT = MomLayout<kNumericsF64>::CNT;
    __shared__ SolveShared sh;
    __shared__ double red[kUpdWaves * NM];
    const int p = xcd_remap(blockIdx.x, gridDim.x);
    PairState& st = w.state[p];
    if (st.phase != kPhaseActive) return;
    const int tid = threadIdx.x;
    const int n = a.src_n[p];
    clear_need(w, p, n, tid, kUpdWG);
    const float4* tgt = a.tgt + a.tgt_off[p];
    float4* X = w.X + (int64_t)p * w.x_stride;
    const int64_t slot0 = (int64_t)p * w.x_stride;
    const KParams& kp = a.kp;
    const bool weighted = kp.huber_delta < INFINITY;
    double mom[NM];
#pragma unroll
    for (int k = 0; k < NM; ++k) mom[k] = 0.0;
    for (int i = tid; i < n; i += kUpdWG) {
        float d2;
        int j;
        load_nn(w, slot0 + i, d2, j);
        if (d2 > kp.max_d2) continue;
        const float4 s = X[i];
        const float4 d = tgt[j];
        const double wt = weighted ? huber_w(d2, kp.huber_delta) : 1.0;
        const double s0 = s.x, s1 = s.y, s2 = s.z;
        const double w0 = wt * (double)d.x, w1 = wt * (double)d.y, w2 = wt * (double)d.z;
        mom[0] += w0 * s0; mom[1] += w0 * s1; mom[2] += w0 * s2;
        mom[3] += w1 * s0; mom[4] += w1 * s1; mom[5] += w1 * s2;
        mom[6] += w2 * s0; mom[7] += w2 * s1; mom[8] += w2 * s2;
        mom[9] += wt * s0; mom[10] += wt * s1; mom[11] += wt * s2;
        mom[12] += w0; mom[13] += w1; mom[14] += w2;
        mom[15] += wt;
        mom[MomLayout<kNumericsF64>::MSE] += (double)d2;
        mom[I_CNT] += 1.0;
    }
    block_sum<NM, kUpdWaves>(mom, red, sh.mom);
    if (tid == 0) solve_pair<kNumericsF64>(sh, st, kp);
    __syncthreads();
    if (sh.flag == 1) return;
    if (!w.defer_xform) transform_pair<kUpdWG>(w, p, n, sh.T_inc, false);
}

// ---------------------------------------------------------------------------------------------
// solo_kernel: one pair's whole registration by one 1024-thread workgroup — the unbatched plan for
// targets of at most kLdsTargets points (C1, C2: the node's per-frame call,
// iterative_closest_point.cpp:510-521), after init_kernel and index_kernel.  The pair's targets and
// boxes are staged into LDS once, and every ICP iteration runs inside the launch, separated by
// workgroup barriers only:
//   test    the cached-neighbour test of every source in sorted-position order (the deferred
//           transformCloud(T_inc), the bounds moved, hit or miss), the misses' search records
//           compacted in that order into the pair's query list — first pass: every source;
//   search  lds_runs<true> over the list (the batched search's run machinery and arithmetic);
//   update  fold passes A and B over (X, nn_t) in index order, the Umeyama solve, hasConverged;
// then the fitness pass (final * input, the test, the misses searched with keys, the sequential
// double sum of Registration::getFitnessScore) and the result row.  Per iteration this removes the
// launches, their boundaries and the target staging of the multi-launch plan; every result is
// bit-identical to it (the same per-query and per-chain arithmetic in the same order).
constexpr int kSoloWG = kLdsWG;
constexpr int kSoloFitChunk = 960;  // fitness chunk: 15 waves fill, wave 0 lane 0 folds
constexpr int kSoloGrp = 4;         // the first pass' sorted positions in flight per thread
// LDS: the pair's target tile stays resident for the whole registration,
// and the search's per-wave state, the update's fold buffers (192-point chunks), the test's bitmap
// and records and the fitness chunks take turns in the 18 KB beside it.  (The other layout — the tile and
// 512-point fold buffers taking turns in one region, the tile restaged from the L2 for each search —
// was the experiment.)
struct SoloTile {
    v4f tl[kLdsTargets];
    alignas(16) float bx[kLdsTargets / kLdsLeaf][6];
    float sbx[kLdsTargets / kLdsLeaf / kSuper][6];
};
struct SoloSearch {  // the search's per-wave state
    unsigned long long best[kLdsWaves][64];
    uint32_t sec[kLdsWaves][64];
    uint16_t items[kLdsWaves][kRing + 64];
};
constexpr int kSoloChunk = 192;  // fold chunk (points)
constexpr int kSoloRow = kSoloChunk + kFoldPad;
struct SoloFold {  // the update
    alignas(16) float buf[2][9][kSoloRow];
    float res[8];
    int32_t cnt[kLdsWaves];
    SolveShared sv;
};
// the test's LDS miss records (24 B each), after the bitmap and its prefixes, in the region they share
constexpr int kSoloRecs = ((int)sizeof(SoloSearch) - 8 * kNeedWords) / 24 & ~15;
struct SoloTest {  // the cached-neighbour test: the miss bitmap, its word prefixes, the miss records
    uint32_t need[kNeedWords];
    int32_t pre[kNeedWords];
    float4 lv[kSoloRecs];
    uint2 lm[kSoloRecs];
};
struct SoloShared {
    SoloTile t;
    union {
        SoloSearch s;
        SoloFold f;
        SoloTest c;
        alignas(16) double fit[2][kSoloFitChunk];  // the fitness sum's chunks (doubles: fold_seq_d)
    } u;
    int32_t wtot[kLdsWaves];  // per-wave counts (the test's misses, the fitness count)
    int32_t mcount;           // the test's LDS record count
};
#define SOLO_F(sh) (sh).u.f
#define SOLO_C(sh) (sh).u.c
#define SOLO_FIT(sh) (sh).u.fit
static_assert(sizeof(SoloShared) <= 160 * 1024, "solo LDS");

// The first pass' query list of the solo plan: every source in sorted-position order (thread t takes
// positions [t * per, (t + 1) * per), kSoloGrp at a time with every load in flight): qv = {X_i as
// init_kernel wrote it, U = +inf}, qm = {source index | sorted position << 14, the target at the same
// relative sorted position — the seed}.  Returns n.
__device__ int solo_first_list(const PairArgs& a, const WorkArgs& w, int p, int n, int m) {
    const int tid = threadIdx.x;
    const int64_t xs0 = (int64_t)p * w.x_stride;
    const float4* X = w.X + xs0;
    const int32_t* sperm = w.sperm + xs0;
    float4* qv = w.qv + xs0;
    uint2* qm = w.qm + xs0;
    const int per = (n + kSoloWG - 1) / kSoloWG;
    const int k0 = min(tid * per, n), k1 = min(k0 + per, n);
    for (int g = k0; g < k1; g += kSoloGrp) {
        int ii[kSoloGrp];
        float4 v[kSoloGrp];
#pragma unroll
        for (int e = 0; e < kSoloGrp; ++e) ii[e] = sperm[min(g + e, k1 - 1)];
#pragma unroll
        for (int e = 0; e < kSoloGrp; ++e) v[e] = X[ii[e]];
#pragma unroll
        for (int e = 0; e < kSoloGrp; ++e) {
            const int k = g + e;
            if (k >= k1) break;
            qv[k] = make_float4(v[e].x, v[e].y, v[e].z, INFINITY);
            qm[k] = make_uint2((uint32_t)ii[e] | ((uint32_t)k << kNtPosShift), (uint32_t)(((int64_t)k * m) / n));
        }
    }
    return n;
}

// The cached-neighbour test of an iteration pass (FROM_SRC = false: X := T_inc X, deferred) or of
// the fitness pass (FROM_SRC: T = final applied to the input): pair_cache_test by the whole
// workgroup, its records in the tile's LDS region; when they overflow it (a pair far from
// converged), the records left in sq / sm are placed at their ranks here.  Returns the list length.
template <bool FROM_SRC>
__device__ int solo_cache_test(const PairArgs& a, const WorkArgs& w, int p, int n, const float (&T)[16],
                               SoloShared& sh, unsigned long long* tk = nullptr) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nwords = (n + 31) >> 5;
    const uint64_t t0 = tk ? __builtin_amdgcn_s_memrealtime() : 0;
    for (int k = tid; k < nwords; k += kSoloWG) SOLO_C(sh).need[k] = 0u;
    if (tid == 0) sh.mcount = 0;
    __syncthreads();
    const int tot = pair_cache_test<kSoloWG, 2, FROM_SRC>(a, w, p, n, T, SOLO_C(sh).need, SOLO_C(sh).pre, SOLO_C(sh).lv,
                                                         SOLO_C(sh).lm, kSoloRecs, &sh.mcount, sh.wtot, FROM_SRC);
    if (tk) {  // debug: the test's own wall, and how many passes overflowed the LDS records
        tk[27] += __builtin_amdgcn_s_memrealtime() - t0;
        tk[28] += tot > kSoloRecs ? 1 : 0;
        tk[29] += tot;
    }
    if (tot <= kSoloRecs) return tot;
    // overflow: every record is in sq / sm (test order), the bitmap still in LDS — word prefixes
    // (wave 0), then each record to its rank
    __syncthreads();
    if (wave == 0) {
        constexpr int kW = kNeedWords / 64;
        int c[kW], sum = 0;
#pragma unroll
        for (int j = 0; j < kW; ++j) {
            const int wd = lane * kW + j;
            c[j] = wd < nwords ? __builtin_popcount(SOLO_C(sh).need[wd]) : 0;
            sum += c[j];
        }
        int incl = sum;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const int o = __shfl_up(incl, off, 64);
            if (lane >= off) incl += o;
        }
        int run = incl - sum;
#pragma unroll
        for (int j = 0; j < kW; ++j) {
            SOLO_C(sh).pre[lane * kW + j] = run;
            run += c[j];
        }
    }
    __syncthreads();
    const int64_t xs0 = (int64_t)p * w.x_stride;
    for (int k = tid; k < tot; k += kSoloWG) {
        const float4 r = w.sq[xs0 + k];
        const uint2 m = w.sm[xs0 + k];
        const uint32_t sp = min(m.y, (uint32_t)(n - 1));
        const int rk = SOLO_C(sh).pre[sp >> 5] + __builtin_popcount(SOLO_C(sh).need[sp >> 5] & ((1u << (sp & 31)) - 1u));
        w.qv[xs0 + rk] = r;
        w.qm[xs0 + rk] = make_uint2((m.x & kNtIdxMask) | (sp << kNtPosShift), m.x >> kNtPosShift);
    }
    return tot;
}

__global__ __launch_bounds__(kSoloWG) void solo_kernel(PairArgs a, WorkArgs w, int iters) {
    __shared__ SoloShared sh;
    const int p = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    PairState& st = w.state[p];
    const KParams& kp = a.kp;
    const int n = uload(a.src_n + p), m = uload(a.tgt_n + p);
    const int64_t xs0 = (int64_t)p * w.x_stride;
    const bool valid = uload(&st.phase) != kPhaseInvalid;
    const int nsb = (((m + kLdsLeaf - 1) / kLdsLeaf) + kSuper - 1) / kSuper;
    const LdsTile tile{sh.t.tl, sh.t.bx, sh.t.sbx};
    RunStats rs;
    auto search = [&](int nlist, bool keys) {
        __syncthreads();  // the list (global, this workgroup's) and the region's previous use
        const v4f* sbg = reinterpret_cast<const v4f*>(w.sbox + (int64_t)p * 2 * w.sb_stride);
        const int sbl = min(lane, nsb - 1);
        v4f isl = sbg[2 * sbl], ish = sbg[2 * sbl + 1];
        lds_runs<true>(tile, sh.u.s.best[wave], sh.u.s.sec[wave], sh.u.s.items[wave], w.qv + xs0, w.qm + xs0, nlist, m, nsb,
                       isl, ish, a, w, p, xs0, w.X + xs0, w.nn_key + xs0, keys, false, rs);
        __syncthreads();
    };
    // debug (plan option phase_ticks = 1): pair 0's phase walls summed over the registration (s_memrealtime,
    // 100 MHz) into ticks[0..9]: staging, test, search, pass A, pass B, solve, fitness test, fitness
    // search, fitness sum, iterations (tools/experiments/solo_phases.py)
    unsigned long long* tk = (w.ticks && p == 0 && tid == 0) ? reinterpret_cast<unsigned long long*>(w.ticks) : nullptr;
    uint64_t tk_last = tk ? __builtin_amdgcn_s_memrealtime() : 0;
    auto tick = [&](int slot) {
        if (!tk) return;
        const uint64_t now = __builtin_amdgcn_s_memrealtime();
        tk[slot] += now - tk_last;
        tk_last = now;
    };
    if (valid) {
        v4f isl, ish;
        stage_tile<kSoloWG>(tile, w, p, nsb, isl, ish);  // (the search reloads its boxes)
        float T[16];
#pragma unroll
        for (int q = 0; q < 16; ++q) T[q] = 0.0f;
        int flag = 0;
        __syncthreads();
        tick(0);
        for (int it = 0; it < iters && flag == 0; ++it) {
            // (first pass: src_order_kernel wrote the records, seeded at the source's kd leaf in the
            // target's tree, when the sources are ordered by it — plan option src_order = 1)
            const int nlist = it > 0 ? solo_cache_test<false>(a, w, p, n, T, sh, tk)
                              : (w.stage_first && src_by_tgt_tree(a, w, p)) ? n : solo_first_list(a, w, p, n, m);
            tick(1);
            search(nlist, false);
            tick(2);
            const FoldIn fin{nullptr, w.X + xs0, w.nn_t + xs0, n};
            fold_pass_a<kSoloWG, kSoloChunk, kSoloRow>(kp, fin, SOLO_F(sh).buf, SOLO_F(sh).res, SOLO_F(sh).cnt, SOLO_F(sh).sv);
            tick(3);
            fold_pass_b<kSoloWG, kSoloChunk, kSoloRow, false>(kp, fin, SOLO_F(sh).buf, SOLO_F(sh).sv);
            tick(4);
            if (tid == 0) solve_pair<kNumericsPCL>(SOLO_F(sh).sv, st, kp);
            __syncthreads();
            tick(5);
            if (tk) tk[9] += 1;
            flag = SOLO_F(sh).sv.flag;
#pragma unroll
            for (int q = 0; q < 16; ++q) T[q] = SOLO_F(sh).sv.T_inc[q];  // the next pass's deferred transform
        }
        // the fitness pass (getFitnessScore after align) and align's output: final * input
        if (kp.compute_fitness || a.aligned) {
            __syncthreads();  // thread 0's final_T
#pragma unroll
            for (int q = 0; q < 16; ++q) T[q] = st.final_T[q];
            if (kp.compute_fitness) {
                const int nlist = solo_cache_test<true>(a, w, p, n, T, sh);
                tick(6);
                search(nlist, true);
                tick(7);
                if (a.aligned) {  // X = final * input (the test wrote it, the search rewrote its misses)
                    __syncthreads();
                    const float4* src = a.src + a.src_off[p];
                    const float4* X = w.X + xs0;
                    for (int i = tid; i < n; i += kSoloWG) {
                        float4 v = X[i];
                        v.w = src[i].w;  // intensity copied through
                        a.aligned[a.src_off[p] + i] = v;
                    }
                }
            } else {
                const float4* src = a.src + a.src_off[p];
                for (int i = tid; i < n; i += kSoloWG) {
                    const float4 s = src[i];
                    float4 o = s;
                    xform_pt(T, s.x, s.y, s.z, o.x, o.y, o.z);
                    a.aligned[a.src_off[p] + i] = o;  // (.w: the input's intensity)
                }
            }
        }
    }
    // Registration::getFitnessScore: the sequential double sum over points with d² <= max_range in
    // index order (wave 0 lane 0 over LDS chunks the other waves fill; points beyond contribute +0)
    // and the exact count (finish_kernel's fold, bit for bit)
    const bool have = valid && kp.compute_fitness && n > 0;
    double fsum = 0.0;
    int fcnt = 0;
    if (have) {
        const NNKey* key = w.nn_key + xs0;
        const int nch = (n + kSoloFitChunk - 1) / kSoloFitChunk;
        auto fill = [&](int c) {
            const int base = c * kSoloFitChunk, len = min(kSoloFitChunk, n - base);
            for (int o = tid - 64; o < len; o += kSoloWG - 64) {
                const float d2 = key_d2(key[base + o]);
                const bool in = (double)d2 <= kp.fit_max_range;
                SOLO_FIT(sh)[c & 1][o] = in ? (double)d2 : 0.0;
                fcnt += in ? 1 : 0;
            }
        };
        if (wave >= 1) fill(0);
        for (int c = 0; c < nch; ++c) {
            __syncthreads();
            if (wave == 0) {
                if (lane == 0) fsum = fold_seq_d(SOLO_FIT(sh)[c & 1], min(kSoloFitChunk, n - c * kSoloFitChunk), fsum);
            } else if (c + 1 < nch) {
                fill(c + 1);
            }
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) fcnt += __shfl_xor(fcnt, off, 64);
        if (lane == 0) sh.wtot[wave] = fcnt;
        __syncthreads();
        fcnt = 0;
        for (int k = 0; k < kLdsWaves; ++k) fcnt += sh.wtot[k];
    }
    tick(8);
    if (tid == 0) {
        Result r;
        for (int k = 0; k < 16; ++k) r.T[k] = st.final_T[k];
        r.fitness = (have && fcnt > 0) ? fsum / fcnt : DBL_MAX;
        r.iterations = st.iterations;
        r.converged = st.phase == kPhaseConverged ? 1 : 0;
        r.status = st.status;
        r.convergence_state = st.conv_state;
        r.n_correspondences = st.ncorr;
        r.reserved = 0;
        a.results[p] = r;
    }
    if (lane == 0) {
        count_add(w.evals, 0, rs.evals);
        count_add(w.evals, 1, rs.tests);
    }
}

// The one corr_kernel launch: the correspondence records of every active pair from its merged keys.
hipError_t launch_corr(const PairArgs& a, const WorkArgs& w, int npairs, int max_n, hipStream_t st) {
    hipLaunchKernelGGL(corr_kernel, dim3((max_n + 255) / 256, npairs), dim3(256), 0, st, a, w);
    return hipGetLastError();
}

hipError_t launch_nn(int q, bool packed, const PairArgs& a, const WorkArgs& w, int npairs, int max_n,
                     int fitness_pass, hipStream_t st) {
    const int per_block = kNNWG * q;
    const dim3 grid((max_n + per_block - 1) / per_block, npairs, w.splits), block(kNNWG);
#define ICP4R_NN_CASE(QQ, PP) hipLaunchKernelGGL((nn_kernel<QQ, PP>), grid, block, 0, st, a, w, fitness_pass)
    if (packed && q >= 2) {
        switch (q) {
            case 2: ICP4R_NN_CASE(2, true); break;
            case 4: ICP4R_NN_CASE(4, true); break;
            case 8: ICP4R_NN_CASE(8, true); break;
            case 16: ICP4R_NN_CASE(16, true); break;
            default: return hipErrorInvalidValue;
        }
    } else {
        switch (q) {
            case 1: ICP4R_NN_CASE(1, false); break;
            case 2: ICP4R_NN_CASE(2, false); break;
            case 4: ICP4R_NN_CASE(4, false); break;
            case 8: ICP4R_NN_CASE(8, false); break;
            case 16: ICP4R_NN_CASE(16, false); break;
            default: return hipErrorInvalidValue;
        }
    }
#undef ICP4R_NN_CASE
    return hipGetLastError();
}

hipError_t launch_nn_lds(const PairArgs& a, const WorkArgs& w, int npairs, int max_n, int fitness_pass, int first,
                         int ncu, hipStream_t st, const NNLdsEvents& ev, int test_fused, int ordered, int pending) {
    // (query records: source index and sorted position in kNtPosShift bits each, every mode)
    if (w.leaf != kLdsLeaf || w.t_stride > kLdsTargets || npairs <= 0 || max_n > (1 << kNtPosShift))
        return hipErrorInvalidValue;
    const bool cache = w.nn_u != nullptr;
    if (cache && (max_n > kCacheMaxN || !w.sq || !w.qv || !w.need || !w.miss_cnt || !w.nn_t || !w.defer_xform))
        return hipErrorInvalidValue;
    if (!w.plist || !w.plist_n || !w.queue || !w.qv || !w.qm) return hipErrorInvalidValue;
    hipError_t e;
    if (cache && !first && !test_fused) {  // (test_fused: the previous fold_update_kernel ran it)
        const int chunks = (max_n + kTestWG * kTestPer - 1) / (kTestWG * kTestPer);
        if (ev.test_start && (e = hipEventRecord(ev.test_start, st)) != hipSuccess) return e;
        hipLaunchKernelGGL(nn_cache_test_kernel, dim3(chunks, npairs), dim3(kTestWG), 0, st, a, w, fitness_pass);
        if (ev.test_stop && (e = hipEventRecord(ev.test_stop, st)) != hipSuccess) return e;
    }
    if (ordered && (first || !cache || fitness_pass || !test_fused)) return hipErrorInvalidValue;
    if (pending && (first || !cache || fitness_pass || !test_fused || !w.lazy_x)) return hipErrorInvalidValue;
    if (!ordered)
        hipLaunchKernelGGL(nn_order_kernel, dim3(1), dim3(kOrderWG), 0, st, a, w, npairs, fitness_pass,
                           (first || !cache) ? 1 : 0, ncu);
    const int grid = npairs < ncu ? npairs : ncu;  // persistent: one workgroup per CU (LDS-bound)
    if (ev.search_start && (e = hipEventRecord(ev.search_start, st)) != hipSuccess) return e;
    if (cache)
        hipLaunchKernelGGL((nn_lds_kernel<true>), dim3(grid), dim3(kLdsWG), 0, st, a, w, fitness_pass, first,
                           test_fused && !first ? 1 : 0, pending);
    else
        hipLaunchKernelGGL((nn_lds_kernel<false>), dim3(grid), dim3(kLdsWG), 0, st, a, w, fitness_pass, first, 0, 0);
    if (ev.search_stop && (e = hipEventRecord(ev.search_stop, st)) != hipSuccess) return e;
    return hipGetLastError();
}

hipError_t launch_nn_tile(const PairArgs& a, const WorkArgs& w, int npairs, int max_n, int max_m, int fitness_pass,
                          int first, int qrun, hipStream_t st, hipEvent_t tile_start, hipEvent_t tile_stop) {
    if (w.leaf != kLdsLeaf || !w.tsort || !w.sperm || max_m >= kTileMaxM || npairs <= 0 || max_n <= 0 ||
        (qrun != 64 && qrun != 32 && qrun != 16 && qrun != 8))
        return hipErrorInvalidValue;
    hipError_t e;
    const int qpart = kLdsWaves * qrun;  // queries per workgroup
    const dim3 grid((max_m + kLdsTargets - 1) / kLdsTargets, (max_n + qpart - 1) / qpart, npairs);
    // one tile: the search kernel seeds, stores and writes the records itself (w.tile_own = 0: the
    // three-launch form, for A/B)
    const bool own = grid.x == 1 && w.tile_own != 0;
    // (w.seed_next: the previous update / fitness_prep_kernel wrote the seeds, except for the first pass)
    if (!own && (first || !w.seed_next))
        hipLaunchKernelGGL(nn_seed_kernel, dim3((max_n + 255) / 256, npairs), dim3(256), 0, st, a, w, fitness_pass,
                           first);
    if (tile_start && (e = hipEventRecord(tile_start, st)) != hipSuccess) return e;
    hipLaunchKernelGGL(nn_tile_kernel, grid, dim3(kLdsWG), 0, st, a, w, fitness_pass, own ? first : -1, qrun);
    if (tile_stop && (e = hipEventRecord(tile_stop, st)) != hipSuccess) return e;
    if (!own && w.corr != nullptr && !fitness_pass && !w.fold_keys)  // records from the merged keys
        return launch_corr(a, w, npairs, max_n, st);
    return hipGetLastError();
}

hipError_t launch_nn_pruned(int q, int chunk_sb, int chunks, const PairArgs& a, const WorkArgs& w, int npairs,
                            int max_n, int fitness_pass, int first, hipStream_t st) {
    const int per_block = kNNWG * q;
    const dim3 grid((max_n + per_block - 1) / per_block, npairs, chunks), block(kNNWG);
    if (chunk_sb < 1 || chunk_sb > 64 || chunks < 1) return hipErrorInvalidValue;
    if (chunks > 1)
        hipLaunchKernelGGL(nn_seed_kernel, dim3((max_n + 255) / 256, npairs), dim3(256), 0, st, a, w, fitness_pass, first);
#define ICP4R_PR_CASE(QQ, BB) \
    hipLaunchKernelGGL((nn_pruned_kernel<QQ, BB>), grid, block, 0, st, a, w, fitness_pass, first, chunk_sb)
    if (w.leaf == 16) {
        switch (q) {
            case 1: ICP4R_PR_CASE(1, 16); break;
            case 2: ICP4R_PR_CASE(2, 16); break;
            case 4: ICP4R_PR_CASE(4, 16); break;
            default: return hipErrorInvalidValue;
        }
    } else if (w.leaf == 32) {
        switch (q) {
            case 1: ICP4R_PR_CASE(1, 32); break;
            case 2: ICP4R_PR_CASE(2, 32); break;
            case 4: ICP4R_PR_CASE(4, 32); break;
            default: return hipErrorInvalidValue;
        }
    } else {
        return hipErrorInvalidValue;
    }
#undef ICP4R_PR_CASE
    if (chunks > 1 && w.corr != nullptr && !fitness_pass)  // records from the merged keys
        return launch_corr(a, w, npairs, max_n, st);
    return hipGetLastError();
}

hipError_t launch_update(const PairArgs& a, const WorkArgs& w, int npairs, int max_n, bool need_corr, hipStream_t st,
                         int tail_test, int order_ncu, bool wide, int silent, int pending) {
    if (silent && pending) return hipErrorInvalidValue;  // (never two silent tails in a row)
    if (order_ncu > 0 && (!tail_test || !w.owork || !w.plist || !w.plist_n || !w.nn_u || a.kp.numerics != kNumericsPCL))
        return hipErrorInvalidValue;
    // (lazy_x: fold_update_kernel's fused tail only — no other update kernel knows a pending pair)
    if (w.lazy_x && (wide || need_corr || w.corr || w.res_update || w.sums_tail || !w.nn_u || !w.defer_xform ||
                     a.kp.numerics != kNumericsPCL))
        return hipErrorInvalidValue;
    if (a.kp.numerics == kNumericsPCL) {
        hipError_t e;
        if (need_corr && (e = launch_corr(a, w, npairs, max_n, st)) != hipSuccess) return e;
        if (wide && !tail_test && order_ncu <= 0 && w.held_update && max_n <= kHeldSmallN)
            hipLaunchKernelGGL((fold_update_held_kernel<3, true>), dim3(npairs), dim3(kWideWG), 0, st, a, w);
        else if (wide && !tail_test && order_ncu <= 0 && w.held_update && max_n <= kHeldMaxN)
            hipLaunchKernelGGL((fold_update_held_kernel<10, false>), dim3(npairs), dim3(kWideWG), 0, st, a, w);
        else if (wide && !tail_test && order_ncu <= 0)
            hipLaunchKernelGGL(fold_update_wide_kernel, dim3(npairs), dim3(kWideWG), 0, st, a, w);
        else if (w.res_update && !need_corr && !w.corr && max_n <= kResMaxN && w.nn_t && w.nn_u && w.defer_xform &&
                 a.kp.huber_delta == INFINITY && a.kp.max_d2 >= FLT_MAX &&
                 !w.sums_tail && (!tail_test || (w.sq && w.sm && w.need && w.miss_cnt)))
            hipLaunchKernelGGL(fold_update_res_kernel, dim3(npairs), dim3(kResWG), 0, st, a, w, tail_test, order_ncu);
        else if (w.lazy_x && pending)
            hipLaunchKernelGGL(fold_update_kernel<true>, dim3(npairs), dim3(kFoldWG), 0, st, a, w, tail_test, order_ncu, 0);
        else
            hipLaunchKernelGGL(fold_update_kernel<false>, dim3(npairs), dim3(kFoldWG), 0, st, a, w, tail_test, order_ncu,
                               (w.lazy_x && tail_test && silent) ? 1 : 0);
    } else {
        hipLaunchKernelGGL(update_f64_kernel, dim3(npairs), dim3(kUpdWG), 0, st, a, w);
    }
    return hipGetLastError();
}

hipError_t launch_solo(const PairArgs& a, const WorkArgs& w, int npairs, int max_n, int iters, hipStream_t st) {
    if (a.kp.numerics != kNumericsPCL || w.leaf != kLdsLeaf || w.t_stride > kLdsTargets || max_n > kCacheMaxN ||
        w.x_stride > kCacheMaxN || !w.tsort || !w.tbox || !w.sbox || !w.sperm || !w.nn_u || !w.nn_t || !w.qv ||
        !w.qm || !w.sq || !w.sm || !w.need || !w.miss_cnt || npairs <= 0 || iters <= 0)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(solo_kernel, dim3(npairs), dim3(kSoloWG), 0, st, a, w, iters);
    return hipGetLastError();
}

}  // namespace icp4r
