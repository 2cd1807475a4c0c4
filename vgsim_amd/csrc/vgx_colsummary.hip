// vgx_colsummary.hip — summaries down the columns of a row-major matrix x[R][N] (f64, or int32 for the event counts of
// vgx_get_incidence) of whole numbers in [0, 2^31), per group of rows:
// count, min, max, exact integer sum and sum of squares, and the order statistics at ranks the caller gives.
// vgx_get_trajectory_summary runs it on the trajectories of the last call where the kernels left them (r_traj is only read),
// vgx_test_column_summary on a matrix it uploads.  Three kernels, all integer work, so no result depends on launch geometry:
//   colsum_transpose  x[perm[slot]][c0 + j] (f64 or int32, a column strided by N elements) -> y[j][slot] (u32), a 64 x 64 tile through LDS,
//                     coalesced on both sides; `perm` lists the member rows group by group, so a (column, group) segment of y is
//                     contiguous;
//   colsum_wave       a segment of at most 64 keys per wavefront, four segments per workgroup: one key per lane, a bitonic network
//                     of cross-lane exchanges, sums by butterfly;
//   colsum_block      a segment of up to VGX_COLSUMMARY_MAX_GROUP keys per workgroup: bitonic sort in LDS, whose exchanges at
//                     distances below 64 run in registers with the same cross-lane steps.
// The columns are processed in chunks so that y never exceeds the scratch bound (VGX_COLSUMMARY_CHUNK_BYTES).
#include "vgx_engine.h"
#include <stdio.h>
#include <stdlib.h>

#pragma GCC visibility push(hidden)

namespace {

constexpr int TILE = 64;                       // transpose tile: 64 slots x 64 columns
constexpr int WAVE_MAX = 64;                   // largest group of the wavefront form
constexpr uint32_t PAD_KEY = 0xFFFFFFFFu;      // sorts behind every value (values are below 2^31)
constexpr size_t DEFAULT_CHUNK_BYTES = (size_t)256 << 20;

struct ColsumOut {                             // device outputs, full width: [G][N] each, stat [G][K][N]
    int64_t *sum;
    uint64_t *sumsq;
    uint32_t *mn, *mx, *stat;
};

// steps j = jfirst, jfirst / 2, .. 1 (all below 64) of the bitonic merge of run length k, on the key of element `idx` held by this lane
// (the 64 lanes hold 64 consecutive elements, lane = idx % 64)
__device__ __forceinline__ uint32_t lane_steps(uint32_t key, unsigned idx, unsigned k, int jfirst) {
    const bool up = (idx & k) == 0;
    for (int j = jfirst; j > 0; j >>= 1) {
        const uint32_t o = (uint32_t)__shfl_xor((int)key, j);
        const bool low = (idx & (unsigned)j) == 0;
        key = (low == up) ? min(key, o) : max(key, o);
    }
    return key;
}

// sorted runs of 64 elements, ascending where (idx & 64) == 0 and descending elsewhere: the first six merges of the network
__device__ __forceinline__ uint32_t lane_sort64(uint32_t key, unsigned idx) {
    for (unsigned k = 2; k <= 64; k <<= 1) key = lane_steps(key, idx, k, (int)(k >> 1));
    return key;
}

struct Acc {                                   // sum of the keys and of their squares (128 bits in two words)
    uint64_t s, lo, hi;
    __device__ __forceinline__ void add(uint32_t v) {
        const uint64_t q = (uint64_t)v * v;
        s += v;
        lo += q;
        hi += lo < q;
    }
    __device__ __forceinline__ void add(const Acc &o) {
        s += o.s;
        lo += o.lo;
        hi += o.hi + (lo < o.lo);
    }
};

__device__ __forceinline__ Acc wave_sum(Acc a) {
    for (int j = 32; j > 0; j >>= 1) {
        Acc o;
        o.s = __shfl_xor((unsigned long long)a.s, j);
        o.lo = __shfl_xor((unsigned long long)a.lo, j);
        o.hi = __shfl_xor((unsigned long long)a.hi, j);
        a.add(o);
    }
    return a;
}

template <typename X>
__global__ __launch_bounds__(256) void colsum_transpose(const X *__restrict__ x, int64_t N, const int64_t *__restrict__ perm, int64_t M,
                                                        int64_t c0, int ncols, uint32_t *__restrict__ y) {
    __shared__ uint32_t tile[TILE][TILE + 1];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int64_t s0 = (int64_t)blockIdx.x * TILE;
    const int j0 = (int)blockIdx.y * TILE;
    for (int i = w; i < TILE; i += 4) {        // a wavefront reads 64 consecutive columns of one member row
        const int64_t s = s0 + i;
        uint32_t v = 0;
        if (s < M && j0 + lane < ncols) v = (uint32_t)x[(size_t)perm[s] * (size_t)N + (size_t)(c0 + j0 + lane)];
        tile[i][lane] = v;
    }
    __syncthreads();
    for (int j = w; j < TILE; j += 4)          // ... and writes 64 consecutive slots of one column
        if (j0 + j < ncols && s0 + lane < M) y[(size_t)(j0 + j) * (size_t)M + (size_t)(s0 + lane)] = tile[lane][j];
}

__global__ __launch_bounds__(256) void colsum_wave(const uint32_t *__restrict__ y, int64_t M, int64_t c0, int ncols, int64_t N,
                                                   const int32_t *__restrict__ glist, int64_t nseg, const int64_t *__restrict__ goff,
                                                   const int32_t *__restrict__ ranks, int K, ColsumOut out) {
    const int lane = threadIdx.x & 63;
    const int64_t seg = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (seg >= nseg) return;                   // (the whole wavefront)
    const int g = glist[seg / ncols];
    const int cl = (int)(seg % ncols);
    const int64_t o = goff[g];
    const int m = (int)(goff[g + 1] - o);      // 1 .. 64
    const uint32_t v = lane < m ? y[(size_t)cl * (size_t)M + (size_t)(o + lane)] : PAD_KEY;
    Acc a = {0, 0, 0};
    if (lane < m) a.add(v);
    a = wave_sum(a);
    const uint32_t key = lane_sort64(v, (unsigned)lane);
    const size_t at = (size_t)g * (size_t)N + (size_t)(c0 + cl);
    const uint32_t lowest = (uint32_t)__shfl((int)key, 0), highest = (uint32_t)__shfl((int)key, m - 1);
    if (lane == 0) {
        out.sum[at] = (int64_t)a.s;
        out.sumsq[2 * at] = a.lo;
        out.sumsq[2 * at + 1] = a.hi;
        out.mn[at] = lowest;
        out.mx[at] = highest;
    }
    for (int k0 = 0; k0 < K; k0 += 64) {
        const int k = k0 + lane;
        const int r = k < K ? ranks[(size_t)g * K + k] : 0;
        const uint32_t q = (uint32_t)__shfl((int)key, r);
        if (k < K) out.stat[((size_t)g * K + k) * (size_t)N + (size_t)(c0 + cl)] = q;
    }
}

__global__ __launch_bounds__(256) void colsum_block(const uint32_t *__restrict__ y, int64_t M, int64_t c0, int64_t N,
                                                    const int32_t *__restrict__ glist, const int64_t *__restrict__ goff,
                                                    const int32_t *__restrict__ ranks, int K, ColsumOut out) {
    extern __shared__ uint32_t keys[];         // [npad]
    __shared__ Acc part[4];
    const int tid = threadIdx.x, lane = tid & 63;
    const int g = glist[blockIdx.y];
    const int cl = (int)blockIdx.x;
    const int64_t o = goff[g];
    const unsigned m = (unsigned)(goff[g + 1] - o);   // 65 .. VGX_COLSUMMARY_MAX_GROUP
    unsigned npad = 128;
    while (npad < m) npad <<= 1;
    const uint32_t *src = y + (size_t)cl * (size_t)M + (size_t)o;
    Acc a = {0, 0, 0};
    for (unsigned i = tid; i < npad; i += 256) {       // (npad is a multiple of 64: a wavefront takes a trip whole or not at all)
        const uint32_t v = i < m ? src[i] : PAD_KEY;
        if (i < m) a.add(v);
        keys[i] = lane_sort64(v, i);
    }
    a = wave_sum(a);
    if (lane == 0) part[tid >> 6] = a;
    __syncthreads();
    for (unsigned k = 128; k <= npad; k <<= 1) {
        for (unsigned j = k >> 1; j >= 64; j >>= 1) {  // exchanges across wavefront runs: through LDS
            for (unsigned t = tid; t < (npad >> 1); t += 256) {
                const unsigned i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), p = i | j;
                const uint32_t lo = keys[i], hi = keys[p];
                if ((lo > hi) == ((i & k) == 0)) {
                    keys[i] = hi;
                    keys[p] = lo;
                }
            }
            __syncthreads();
        }
        for (unsigned i = tid; i < npad; i += 256) keys[i] = lane_steps(keys[i], i, k, 32);   // ... inside them: in registers
        __syncthreads();
    }
    const size_t at = (size_t)g * (size_t)N + (size_t)(c0 + cl);
    if (tid == 0) {
        a = part[0];
        a.add(part[1]);
        a.add(part[2]);
        a.add(part[3]);
        out.sum[at] = (int64_t)a.s;
        out.sumsq[2 * at] = a.lo;
        out.sumsq[2 * at + 1] = a.hi;
        out.mn[at] = keys[0];
        out.mx[at] = keys[m - 1];
    }
    for (int k = tid; k < K; k += 256) out.stat[((size_t)g * K + k) * (size_t)N + (size_t)(c0 + cl)] = keys[ranks[(size_t)g * K + k]];
}

struct DevMem {                                // device allocations of one call, freed when it returns
    std::vector<void *> all;
    ~DevMem() {
        for (void *p : all) (void)hipFree(p);
    }
    template <typename T>
    hipError_t get(T **p, size_t n) {
        hipError_t rc = hipMalloc((void **)p, std::max<size_t>(n, 1) * sizeof(T));
        if (rc == hipSuccess) all.push_back(*p);
        return rc;
    }
};

#define CS_HIP(call)                                                                 \
    do {                                                                             \
        hipError_t err__ = (call);                                                   \
        if (err__ != hipSuccess) {                                                   \
            err = std::string(what) + ": " #call ": " + hipGetErrorString(err__);    \
            return VGX_ERR_HIP;                                                      \
        }                                                                            \
    } while (0)

double ms_since(std::chrono::steady_clock::time_point t0) {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

// The summary of the matrix x[R][N] into the host arrays of `io`: x is a device matrix, or (x_on_host) a host matrix that is uploaded
// once the arguments have passed.  `what` prefixes every message.
template <typename X>
int column_summary(const char *what, const X *x, bool x_on_host, int64_t R, int64_t N, vgx_traj_summary_io *io, hipStream_t stream,
                   std::string &err) {
    const auto wall0 = std::chrono::steady_clock::now();
    const int64_t G = io->G, K = io->K;
    if (R < 0 || N < 1 || G < 1 || K < 0 || G > INT32_MAX || K > INT32_MAX || (R && !io->group_of) || (K && (!io->ranks || !io->stat)) ||
        !io->count || !io->sum || !io->sumsq || !io->min || !io->max) {
        err = std::string(what) + ": bad argument";
        return VGX_ERR_ARG;
    }
    // members of every group, in replicate order; perm lists them group by group
    std::vector<int64_t> goff((size_t)G + 1, 0);
    for (int64_t r = 0; r < R; r++) {
        const int64_t g = io->group_of[r];
        if (g < -1 || g >= G) {
            err = std::string(what) + ": group_of[" + std::to_string(r) + "] = " + std::to_string(g) + " is outside [-1, " + std::to_string(G) + ")";
            return VGX_ERR_ARG;
        }
        if (g >= 0) goff[(size_t)g + 1]++;
    }
    std::vector<int32_t> small, big;
    int64_t max_big = 0;
    for (int64_t g = 0; g < G; g++) {
        const int64_t m = goff[(size_t)g + 1];
        io->count[g] = m;
        if (m > VGX_COLSUMMARY_MAX_GROUP) {
            err = std::string(what) + ": group " + std::to_string(g) + " has " + std::to_string(m) + " members; at most " +
                  std::to_string((int64_t)VGX_COLSUMMARY_MAX_GROUP) + " can be sorted in a workgroup's LDS";
            return VGX_ERR_ARG;
        }
        for (int64_t k = 0; k < K && m > 0; k++) {
            const int64_t rk = io->ranks[g * K + k];
            if (rk < 0 || rk >= m) {
                err = std::string(what) + ": rank " + std::to_string(rk) + " of group " + std::to_string(g) + " is outside [0, " + std::to_string(m) + ")";
                return VGX_ERR_ARG;
            }
        }
        if (m > WAVE_MAX) big.push_back((int32_t)g), max_big = std::max(max_big, m);
        else if (m > 0) small.push_back((int32_t)g);
        goff[(size_t)g + 1] += goff[(size_t)g];
    }
    if (big.size() > 65535) {
        err = std::string(what) + ": more than 65535 groups of over " + std::to_string(WAVE_MAX) + " members";
        return VGX_ERR_ARG;
    }
    const int64_t M = goff[(size_t)G];
    std::vector<int64_t> perm((size_t)std::max<int64_t>(M, 1)), fill(goff.begin(), goff.end() - 1);
    for (int64_t r = 0; r < R; r++)
        if (io->group_of[r] >= 0) perm[(size_t)fill[(size_t)io->group_of[r]]++] = r;
    std::vector<int32_t> ranks32((size_t)std::max<int64_t>(G * K, 1), 0);
    for (int64_t i = 0; i < G * K; i++)
        if (io->count[i / K] > 0) ranks32[(size_t)i] = (int32_t)io->ranks[i];

    // columns per chunk: whole tiles, y within the scratch bound (one tile of columns at the least)
    size_t chunk_bytes = DEFAULT_CHUNK_BYTES;
    if (const char *s = getenv("VGX_COLSUMMARY_CHUNK_BYTES")) chunk_bytes = (size_t)std::max<long long>(atoll(s), 1);
    int64_t chunk = (int64_t)(chunk_bytes / ((size_t)std::max<int64_t>(M, 1) * 4)) / TILE * TILE;
    chunk = std::min<int64_t>(std::max<int64_t>(chunk, TILE), (N + TILE - 1) / TILE * TILE);
    chunk = std::min<int64_t>(chunk, (int64_t)65535 * TILE);
    // (the wavefront form's grid: four segments per workgroup, kept below 2^29 workgroups whatever the override says)
    if (!small.empty()) chunk = std::max<int64_t>(std::min<int64_t>(chunk, (((int64_t)1 << 31) / (int64_t)small.size()) / TILE * TILE), TILE);

    const auto copy0 = std::chrono::steady_clock::now();
    const size_t GN = (size_t)G * (size_t)N;
    DevMem dm;
    int64_t *d_perm = nullptr, *d_goff = nullptr;
    int32_t *d_small = nullptr, *d_big = nullptr, *d_ranks = nullptr;
    uint32_t *d_y = nullptr;
    ColsumOut out{};
    const X *d_x = x;
    if (x_on_host) {
        X *up = nullptr;
        CS_HIP(dm.get(&up, (size_t)(R * N)));
        if (R) CS_HIP(hipMemcpyAsync(up, x, (size_t)(R * N) * sizeof(X), hipMemcpyHostToDevice, stream));
        d_x = up;
    }
    CS_HIP(dm.get(&d_perm, perm.size()));
    CS_HIP(dm.get(&d_goff, goff.size()));
    CS_HIP(dm.get(&d_small, small.size()));
    CS_HIP(dm.get(&d_big, big.size()));
    CS_HIP(dm.get(&d_ranks, ranks32.size()));
    CS_HIP(dm.get(&d_y, (size_t)chunk * (size_t)std::max<int64_t>(M, 1)));
    CS_HIP(dm.get(&out.sum, GN));
    CS_HIP(dm.get(&out.sumsq, 2 * GN));
    CS_HIP(dm.get(&out.mn, GN));
    CS_HIP(dm.get(&out.mx, GN));
    CS_HIP(dm.get(&out.stat, GN * (size_t)K));
    CS_HIP(hipMemcpyAsync(d_perm, perm.data(), perm.size() * 8, hipMemcpyHostToDevice, stream));
    CS_HIP(hipMemcpyAsync(d_goff, goff.data(), goff.size() * 8, hipMemcpyHostToDevice, stream));
    if (!small.empty()) CS_HIP(hipMemcpyAsync(d_small, small.data(), small.size() * 4, hipMemcpyHostToDevice, stream));
    if (!big.empty()) CS_HIP(hipMemcpyAsync(d_big, big.data(), big.size() * 4, hipMemcpyHostToDevice, stream));
    CS_HIP(hipMemcpyAsync(d_ranks, ranks32.data(), ranks32.size() * 4, hipMemcpyHostToDevice, stream));
    // an empty group's outputs are zero
    CS_HIP(hipMemsetAsync(out.sum, 0, GN * 8, stream));
    CS_HIP(hipMemsetAsync(out.sumsq, 0, GN * 16, stream));
    CS_HIP(hipMemsetAsync(out.mn, 0, GN * 4, stream));
    CS_HIP(hipMemsetAsync(out.mx, 0, GN * 4, stream));
    if (K) CS_HIP(hipMemsetAsync(out.stat, 0, GN * (size_t)K * 4, stream));
    CS_HIP(hipStreamSynchronize(stream));
    double copy_ms = ms_since(copy0);

    unsigned npad = 128;
    while ((int64_t)npad < max_big) npad <<= 1;
    const size_t lds = big.empty() ? 0 : (size_t)npad * 4;
    if (lds > 48 * 1024) CS_HIP(hipFuncSetAttribute((const void *)colsum_block, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    CS_HIP(hipEventCreate(&ev0));
    if (hipEventCreate(&ev1) != hipSuccess) {
        (void)hipEventDestroy(ev0);
        err = std::string(what) + ": hipEventCreate failed";
        return VGX_ERR_HIP;
    }
    hipError_t rc = hipEventRecord(ev0, stream);
    io->passes = 0;
    for (int64_t c0 = 0; c0 < N && M > 0 && rc == hipSuccess; c0 += chunk, io->passes++) {
        const int ncols = (int)std::min<int64_t>(chunk, N - c0);
        hipLaunchKernelGGL(colsum_transpose<X>, dim3((unsigned)((M + TILE - 1) / TILE), (unsigned)((ncols + TILE - 1) / TILE)), dim3(256), 0, stream,
                           d_x, N, d_perm, M, c0, ncols, d_y);
        if (!small.empty()) {
            const int64_t nseg = (int64_t)small.size() * ncols;
            hipLaunchKernelGGL(colsum_wave, dim3((unsigned)((nseg + 3) / 4)), dim3(256), 0, stream, d_y, M, c0, ncols, N, d_small, nseg, d_goff,
                               d_ranks, (int)K, out);
        }
        if (!big.empty())
            hipLaunchKernelGGL(colsum_block, dim3((unsigned)ncols, (unsigned)big.size()), dim3(256), lds, stream, d_y, M, c0, N, d_big, d_goff,
                               d_ranks, (int)K, out);
        rc = hipGetLastError();
    }
    if (rc == hipSuccess) rc = hipEventRecord(ev1, stream);
    if (rc == hipSuccess) rc = hipEventSynchronize(ev1);
    float kernel_ms = 0.f;
    if (rc == hipSuccess) rc = hipEventElapsedTime(&kernel_ms, ev0, ev1);
    (void)hipEventDestroy(ev0);
    (void)hipEventDestroy(ev1);
    if (rc != hipSuccess) {
        err = std::string(what) + ": " + hipGetErrorString(rc);
        return VGX_ERR_HIP;
    }

    const auto copy1 = std::chrono::steady_clock::now();
    CS_HIP(hipMemcpy(io->sum, out.sum, GN * 8, hipMemcpyDeviceToHost));
    CS_HIP(hipMemcpy(io->sumsq, out.sumsq, GN * 16, hipMemcpyDeviceToHost));
    std::vector<uint32_t> h32(GN * (size_t)std::max<int64_t>(K, 1));
    const struct { const uint32_t *src; int64_t *dst; size_t n; } narrow[3] = {{out.mn, io->min, GN}, {out.mx, io->max, GN}, {out.stat, io->stat, GN * (size_t)K}};
    for (const auto &c : narrow) {
        if (!c.n) continue;
        CS_HIP(hipMemcpy(h32.data(), c.src, c.n * 4, hipMemcpyDeviceToHost));
        for (size_t i = 0; i < c.n; i++) c.dst[i] = (int64_t)h32[i];
    }
    io->ms[0] = kernel_ms;
    io->ms[1] = copy_ms + ms_since(copy1);
    io->ms[2] = ms_since(wall0);
    return VGX_OK;
}

}  // namespace

#pragma GCC visibility pop

// the same kernels on a device int32 matrix (vgx_get_incidence: the block of event counts where the counting kernel left it)
extern "C" __attribute__((visibility("hidden"))) int vgxi_column_summary_i32(const char *what, const int32_t *x, int64_t R, int64_t N,
                                                                             vgx_traj_summary_io *io, hipStream_t stream, char *errbuf,
                                                                             int64_t errcap) {
    std::string err;
    const int rc = io ? column_summary<int32_t>(what, x, false, R, N, io, stream, err) : VGX_ERR_ARG;
    if (rc && errbuf && errcap > 0) snprintf(errbuf, (size_t)errcap, "%s", err.c_str());
    return rc;
}

extern "C" int vgx_get_trajectory_summary(vgx_engine *e, vgx_traj_summary_io *io) {
    if (!e || !io) return VGX_ERR_ARG;
    if (e->traj_points <= 0) return fail(e, VGX_ERR_ARG, "vgx_get_trajectory_summary: the last call recorded none");
    for (int64_t pn = 0; pn < e->d.popNum; pn++)
        if (e->sizes[(size_t)pn] >= ((int64_t)1 << 31)) return fail(e, VGX_ERR_ARG, "vgx_get_trajectory_summary: population sizes of 2^31 or more");
    HIPCHECK(e, hipSetDevice(e->device));
    std::string err;
    const int rc = column_summary("vgx_get_trajectory_summary", (const double *)e->r_traj.p, false, e->R, e->traj_points * e->d.popNum * 2, io, e->stream, err);
    return rc ? fail(e, rc, err) : VGX_OK;
}

extern "C" int vgx_test_column_summary(const double *x, int64_t R, int64_t N, vgx_traj_summary_io *io, char *errbuf, int64_t errcap) {
    std::string err;
    int rc = VGX_OK;
    if (!x || !io || R < 0 || N < 1) {
        err = "vgx_test_column_summary: bad argument";
        rc = VGX_ERR_ARG;
    }
    for (int64_t i = 0; !rc && i < R * N; i++)
        if (!(x[i] >= 0.0 && x[i] < 2147483648.0 && x[i] == std::floor(x[i]))) {
            err = "vgx_test_column_summary: x[" + std::to_string(i / N) + "][" + std::to_string(i % N) + "] is not a whole number in [0, 2^31)";
            rc = VGX_ERR_ARG;
        }
    if (!rc) rc = column_summary("vgx_test_column_summary", x, true, R, N, io, nullptr, err);
    if (rc && errbuf && errcap > 0) snprintf(errbuf, (size_t)errcap, "%s", err.c_str());
    return rc;
}
