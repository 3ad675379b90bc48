// Pauli expectation values for CDNA4: one read-only stream of the state for a
// whole batch of Pauli strings.
//
//   <psi|P|psi> = Re( i^nY  sum_i (-1)^popcount(i & z) conj(a[i ^ x]) a[i] )
//
// with x the positions carrying X or Y, z those carrying Z or Y.  The pairs
// (i, i ^ x) make the sum real when popcount(x & z) (the number of Y's) is even
// and imaginary when it is odd, so each term accumulates one fp64 value.
//
// Three kernels, all deterministic like kernels_reduce.hip (no float atomics:
// wave reduction, one slot per (workgroup, term), single-workgroup finish):
//  * pauliTileKernel: the hot path.  A workgroup stages a tile of 2^12
//    amplitudes in LDS -- the lowest 5 positions (256- / 128-byte runs of
//    fp64 / fp32), the batch's other X / Y positions, padded with the next
//    lowest -- and evaluates up to 16 terms on it: per term and element one
//    LDS read of the partner (tile index ^ x, a lane permutation: no bank
//    conflicts) and three fp64 operations.  The next tile's loads are in
//    flight meanwhile (register software pipeline, as innerPermKernel), and
//    two workgroups fit a CU (64 KiB of LDS each for fp64).
//  * pauliGenericKernel: any x (chunks smaller than a tile, strings with X / Y
//    on more positions than a tile holds); grid-stride, the chunk re-read per
//    term.
//  * pauliDensKernel: Tr(P rho) over the 2^n elements rho(i, i ^ x), in the
//    style of densDiagKernel.
// The reference computes one term at a time through a clone of the register
// (v3 statevec_calcExpecPauliProd: clone, apply the Paulis, inner product).
#include "qa_hip.h"
#include "quest_amd.h"

#include <algorithm>
#include <type_traits>

namespace qa {
namespace hipk {

namespace {

constexpr int kThreads = 256;
constexpr int kMaxBlocks = 2048;
constexpr int kMaxTerms = QUEST_PAULI_MAX_TERMS_PER_PASS;
constexpr int kTileBits = QUEST_PAULI_TILE_QUBITS;
constexpr int kLowBits = QUEST_PAULI_TILE_LOW_QUBITS;
static_assert(kTileBits == 12 && kMaxTerms <= 32 && kLowBits >= 2, "tile shape of pauliTileKernel");

double* g_part = nullptr;     // 2 * kMaxTerms * kMaxBlocks doubles
double* g_out = nullptr;      // 2 * kMaxTerms doubles (device)
double* g_outHost = nullptr;  // the same, pinned

void ensureScratch() {
    if (g_part) return;
    QA_HIP_CHECK(hipMalloc(&g_part, sizeof(double) * 2 * kMaxTerms * kMaxBlocks));
    QA_HIP_CHECK(hipMalloc(&g_out, sizeof(double) * 2 * kMaxTerms));
    QA_HIP_CHECK(hipHostMalloc(&g_outHost, sizeof(double) * 2 * kMaxTerms, hipHostMallocDefault));
}

__device__ __forceinline__ double waveSum(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// sum over the block; result valid in thread 0
__device__ __forceinline__ double blockSum(double v) {
    __shared__ double sh[kThreads / 64];
    v = waveSum(v);
    const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
    __syncthreads();
    if (l == 0) sh[w] = v;
    __syncthreads();
    double r = 0;
    if (threadIdx.x == 0)
        for (int k = 0; k < kThreads / 64; k++) r += sh[k];
    return r;
}

struct PauliTileArgs {
    int nOut;                  // positions outside the tile (L - kTileBits)
    int nTerms;
    unsigned odd;              // bit t: term t has an odd number of Y's (its sum is imaginary)
    signed char tpos[16];      // tile bit -> physical position, ascending (tpos[b] == b for b < kLowBits)
    signed char opos[48];      // the other positions, ascending
    unsigned xl[kMaxTerms], zl[kMaxTerms];   // the terms' masks in tile bits
    unsigned long long zo[kMaxTerms];        // z on the positions outside the tile (physical)
};

// (two workgroups a CU -- one loads while the other computes: 2 waves per SIMD, 256 registers each)
template <typename T>
__global__ __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(2))) void pauliTileKernel(const T* __restrict__ re, const T* __restrict__ im,
                                                            PauliTileArgs pa, double* __restrict__ part) {
    using V = typename Vec16<T>::type;
    using P = typename std::conditional<sizeof(T) == 8, double2, float2>::type;   // (re, im) of one amplitude
    constexpr int VN = Vec16<T>::n;
    constexpr int E = 1 << kTileBits;
    constexpr int NU = E / VN / kThreads;   // 16-byte units a thread loads per array
    constexpr int NE = E / kThreads;        // tile elements a thread owns: tid + kThreads k
    __shared__ P tile[E];
    const int tid = threadIdx.x;
    // unit tid + kThreads k holds the tile elements VN (tid + kThreads k) + j, j < VN: consecutive in
    // memory (tile bits below kLowBits are positions 0 ..)
    const unsigned long long laneOff = scatterBits((unsigned long long)(tid * VN), pa.tpos, kTileBits);
    unsigned long long unitOff[NU];
#pragma unroll
    for (int k = 0; k < NU; k++)
        unitOff[k] = scatterBits((unsigned long long)(k * kThreads * VN), pa.tpos, kTileBits);
    const long long tiles = 1ll << pa.nOut;
    // the next tile is loaded while this one is reduced (software pipeline:
    // one tile in registers ahead)
    V nr[NU], ni[NU];
    auto load = [&](long long tt) {
        const unsigned long long base = scatterBits((unsigned long long)tt, pa.opos, pa.nOut);
#pragma unroll
        for (int k = 0; k < NU; k++) {
            nr[k] = streamLoad(reinterpret_cast<const V*>(re + (base | laneOff | unitOff[k])));
            ni[k] = streamLoad(reinterpret_cast<const V*>(im + (base | laneOff | unitOff[k])));
        }
    };
    double acc[kMaxTerms];
#pragma unroll
    for (int u = 0; u < kMaxTerms; u++) acc[u] = 0;
    if ((long long)blockIdx.x < tiles) load(blockIdx.x);
    for (long long t = blockIdx.x; t < tiles; t += gridDim.x) {
#pragma unroll
        for (int k = 0; k < NU; k++) {
            const T* a = reinterpret_cast<const T*>(&nr[k]);
            const T* b = reinterpret_cast<const T*>(&ni[k]);
#pragma unroll
            for (int j = 0; j < VN; j++) {
                P p;
                p.x = a[j];
                p.y = b[j];
                tile[VN * (tid + kThreads * k) + j] = p;
            }
        }
        const unsigned long long base = scatterBits((unsigned long long)t, pa.opos, pa.nOut);
        if (t + gridDim.x < tiles) load(t + gridDim.x);
        __syncthreads();
        P own[NE];
#pragma unroll
        for (int k = 0; k < NE; k++) own[k] = tile[tid + kThreads * k];
        for (int s = 0; s < pa.nTerms; s++) {
            const unsigned xl = pa.xl[s], zl = pa.zl[s];
            const unsigned xh = xl >> 8, zh = zl >> 8;   // the masks' bits in k
            double sum = 0;
            if (xl == 0) {   // Z / I only: the partner is the element itself
#pragma unroll
                for (int k = 0; k < NE; k++) {
                    const double sg = (__popc(k & zh) & 1) ? -1.0 : 1.0;
                    const double v = (double)own[k].x * own[k].x + (double)own[k].y * own[k].y;
                    sum = fma(sg, v, sum);
                }
            } else {
                const int pl = tid ^ (int)(xl & (kThreads - 1));   // lanes permuted: conflict-free like own[]
                if ((pa.odd >> s) & 1) {
#pragma unroll
                    for (int k = 0; k < NE; k++) {
                        const P p = tile[pl + kThreads * (k ^ (int)xh)];
                        const double sg = (__popc(k & zh) & 1) ? -1.0 : 1.0;
                        const double v = (double)p.x * own[k].y - (double)p.y * own[k].x;   // Im conj(p) a
                        sum = fma(sg, v, sum);
                    }
                } else {
#pragma unroll
                    for (int k = 0; k < NE; k++) {
                        const P p = tile[pl + kThreads * (k ^ (int)xh)];
                        const double sg = (__popc(k & zh) & 1) ? -1.0 : 1.0;
                        const double v = (double)p.x * own[k].x + (double)p.y * own[k].y;   // Re conj(p) a
                        sum = fma(sg, v, sum);
                    }
                }
            }
            // the lane's tile bits and the tile's own index bits under z
            if ((__popc((unsigned)tid & zl) + __popcll(base & pa.zo[s])) & 1) sum = -sum;
#pragma unroll
            for (int u = 0; u < kMaxTerms; u++)
                if (u == s) acc[u] += sum;
        }
        __syncthreads();
    }
    // per term: wave sums through the (now free) tile, one slot per workgroup
    double* red = reinterpret_cast<double*>(tile);
    const int w = tid >> 6, l = tid & 63;
#pragma unroll
    for (int u = 0; u < kMaxTerms; u++) {
        const double v = waveSum(acc[u]);
        if (l == 0) red[u * (kThreads / 64) + w] = v;
    }
    __syncthreads();
    if (tid < pa.nTerms) {
        double v = 0;
#pragma unroll
        for (int k = 0; k < kThreads / 64; k++) v += red[tid * (kThreads / 64) + k];
        part[(long long)tid * kMaxBlocks + blockIdx.x] = v;
    }
}

struct PauliTerms {
    int nTerms;
    unsigned odd;
    unsigned long long x[kMaxTerms], z[kMaxTerms];
};

// any x below n: vector loads where x has no bit inside a 16-byte vector
template <typename T>
__global__ __launch_bounds__(kThreads) void pauliGenericKernel(const T* __restrict__ re, const T* __restrict__ im,
                                                               long long n, PauliTerms pt,
                                                               double* __restrict__ part) {
    using V = typename Vec16<T>::type;
    constexpr int VN = Vec16<T>::n;
    const long long stride = (long long)gridDim.x * blockDim.x;
    const long long first = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    for (int s = 0; s < pt.nTerms; s++) {
        const long long x = (long long)pt.x[s];
        const unsigned long long z = pt.z[s];
        const bool odd = (pt.odd >> s) & 1;
        double acc = 0;
        if ((x & (VN - 1)) == 0 && n >= VN) {
            for (long long u = first; u < n / VN; u += stride) {
                const long long i = u * VN, j = i ^ x;
                const V ar = *reinterpret_cast<const V*>(re + i), ai = *reinterpret_cast<const V*>(im + i);
                const V br = *reinterpret_cast<const V*>(re + j), bi = *reinterpret_cast<const V*>(im + j);
                const T *pa = reinterpret_cast<const T*>(&ar), *pb = reinterpret_cast<const T*>(&ai);
                const T *pc = reinterpret_cast<const T*>(&br), *pd = reinterpret_cast<const T*>(&bi);
#pragma unroll
                for (int e = 0; e < VN; e++) {
                    const double v = odd ? (double)pc[e] * pb[e] - (double)pd[e] * pa[e]
                                         : (double)pc[e] * pa[e] + (double)pd[e] * pb[e];
                    acc += (__popcll((unsigned long long)(i + e) & z) & 1) ? -v : v;
                }
            }
        } else {
            for (long long i = first; i < n; i += stride) {
                const long long j = i ^ x;
                const double v = odd ? (double)re[j] * im[i] - (double)im[j] * re[i]
                                     : (double)re[j] * re[i] + (double)im[j] * im[i];
                acc += (__popcll((unsigned long long)i & z) & 1) ? -v : v;
            }
        }
        const double r = blockSum(acc);
        if (threadIdx.x == 0) part[(long long)s * kMaxBlocks + blockIdx.x] = r;
    }
}

struct PauliDensArgs {
    int nq, nTerms;
    unsigned long long rowOffs[32], colOffs[32];
    unsigned long long x[kMaxTerms], z[kMaxTerms];
};

// per term: sum over rows r of (-1)^popcount(r & z) rho(r, r ^ x), elements of this chunk only
template <typename T>
__global__ __launch_bounds__(kThreads) void pauliDensKernel(const T* __restrict__ re, const T* __restrict__ im,
                                                            long long chunkAmps, long long chunkStart,
                                                            PauliDensArgs da, double* __restrict__ part) {
    const long long dim = 1ll << da.nq;
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (int s = 0; s < da.nTerms; s++) {
        double sr = 0, si = 0;
        for (long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x; r < dim; r += stride) {
            const long long c = r ^ (long long)da.x[s];
            long long p = 0;
            for (int b = 0; b < da.nq; b++) {
                if ((r >> b) & 1) p |= (long long)da.rowOffs[b];
                if ((c >> b) & 1) p |= (long long)da.colOffs[b];
            }
            p -= chunkStart;
            if (p >= 0 && p < chunkAmps) {
                const bool neg = __popcll((unsigned long long)r & da.z[s]) & 1;
                sr += neg ? -(double)re[p] : (double)re[p];
                si += neg ? -(double)im[p] : (double)im[p];
            }
        }
        const double s0 = blockSum(sr);
        const double s1 = blockSum(si);
        if (threadIdx.x == 0) {
            part[(long long)(2 * s) * kMaxBlocks + blockIdx.x] = s0;
            part[(long long)(2 * s + 1) * kMaxBlocks + blockIdx.x] = s1;
        }
    }
}

__global__ __launch_bounds__(kThreads) void pauliFinishKernel(const double* __restrict__ part, int nb, int nvals,
                                                              double* __restrict__ out) {
    for (int v = 0; v < nvals; v++) {
        double acc = 0;
        for (int i = threadIdx.x; i < nb; i += blockDim.x) acc += part[(long long)v * kMaxBlocks + i];
        const double s = blockSum(acc);
        if (threadIdx.x == 0) out[v] = s;
    }
}

void finish(int nb, int nvals) {
    hipLaunchKernelGGL(pauliFinishKernel, dim3(1), dim3(kThreads), 0, stream(), g_part, nb, nvals, g_out);
    QA_HIP_CHECK(hipGetLastError());
    QA_HIP_CHECK(hipMemcpyAsync(g_outHost, g_out, sizeof(double) * nvals, hipMemcpyDeviceToHost, stream()));
    syncStream();
}

}  // namespace

void reducePauli(const real* re, const real* im, int L, int nTerms, const u64* x, const u64* z, double* out) {
    if (nTerms < 1 || nTerms > kMaxTerms) fatal("reducePauli", "term count out of range", __FILE__, __LINE__);
    ensureScratch();
    const u64 lowMask = (1ull << kLowBits) - 1;
    u64 hi = 0;
    unsigned odd = 0;
    for (int t = 0; t < nTerms; t++) {
        if (x[t] >> L) fatal("reducePauli", "X / Y on a position outside the chunk", __FILE__, __LINE__);
        hi |= x[t] & ~lowMask;
        if (__builtin_popcountll(x[t] & z[t]) & 1) odd |= 1u << t;
    }
    int nb;
    if (L >= kTileBits && __builtin_popcountll(hi) <= kTileBits - kLowBits) {
        // tile positions: the low ones, the batch's other X / Y positions, the next lowest
        u64 tileMask = lowMask | hi;
        for (int p = kLowBits; __builtin_popcountll(tileMask) < kTileBits; p++) tileMask |= 1ull << p;
        PauliTileArgs pa = {};
        pa.nOut = L - kTileBits;
        pa.nTerms = nTerms;
        pa.odd = odd;
        int nt = 0, no = 0;
        for (int p = 0; p < L; p++) {
            if ((tileMask >> p) & 1)
                pa.tpos[nt++] = (signed char)p;
            else
                pa.opos[no++] = (signed char)p;
        }
        if (nt != kTileBits || no != pa.nOut) fatal("reducePauli", "tile positions", __FILE__, __LINE__);
        for (int t = 0; t < nTerms; t++) {
            for (int b = 0; b < kTileBits; b++) {
                if ((x[t] >> pa.tpos[b]) & 1) pa.xl[t] |= 1u << b;
                if ((z[t] >> pa.tpos[b]) & 1) pa.zl[t] |= 1u << b;
            }
            pa.zo[t] = z[t] & ~tileMask;
        }
        const long long tiles = 1ll << pa.nOut;
        nb = (int)std::min<long long>(tiles, std::min(kMaxBlocks, 2 * numCUs()));
        hipLaunchKernelGGL(pauliTileKernel<real>, dim3(nb), dim3(kThreads), 0, stream(), re, im, pa, g_part);
    } else {
        PauliTerms pt = {};
        pt.nTerms = nTerms;
        pt.odd = odd;
        for (int t = 0; t < nTerms; t++) {
            pt.x[t] = x[t];
            pt.z[t] = z[t];
        }
        const long long n = 1ll << L;
        const long long work = n / Vec16<real>::n;
        nb = (int)std::min<long long>(kMaxBlocks, std::max<long long>(1, (work + kThreads * 4 - 1) / (kThreads * 4)));
        hipLaunchKernelGGL(pauliGenericKernel<real>, dim3(nb), dim3(kThreads), 0, stream(), re, im, n, pt, g_part);
    }
    QA_HIP_CHECK(hipGetLastError());
    finish(nb, nTerms);
    for (int t = 0; t < nTerms; t++) {
        const bool o = (odd >> t) & 1;
        out[2 * t] = o ? 0.0 : g_outHost[t];
        out[2 * t + 1] = o ? g_outHost[t] : 0.0;
    }
}

void reduceDensPauli(const real* re, const real* im, i64 chunkAmps, const u64* rowOffs, const u64* colOffs, int nq,
                     i64 chunkStart, int nTerms, const u64* x, const u64* z, double* out) {
    if (nTerms < 1 || nTerms > kMaxTerms || nq > 32)
        fatal("reduceDensPauli", "term or qubit count out of range", __FILE__, __LINE__);
    ensureScratch();
    PauliDensArgs da = {};
    da.nq = nq;
    da.nTerms = nTerms;
    for (int j = 0; j < nq; j++) {
        da.rowOffs[j] = rowOffs[j];
        da.colOffs[j] = colOffs[j];
    }
    for (int t = 0; t < nTerms; t++) {
        da.x[t] = x[t];
        da.z[t] = z[t];
    }
    const long long dim = 1ll << nq;
    const int nb = (int)std::min<long long>(kMaxBlocks, std::max<long long>(1, (dim + kThreads * 4 - 1) / (kThreads * 4)));
    hipLaunchKernelGGL(pauliDensKernel<real>, dim3(nb), dim3(kThreads), 0, stream(), re, im, (long long)chunkAmps,
                       (long long)chunkStart, da, g_part);
    QA_HIP_CHECK(hipGetLastError());
    finish(nb, 2 * nTerms);
    for (int v = 0; v < 2 * nTerms; v++) out[v] = g_outHost[v];
}

}  // namespace hipk
}  // namespace qa
