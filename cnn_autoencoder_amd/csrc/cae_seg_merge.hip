// The second launches of the slide metrics (cae_seg_metrics.hpp): block partials -> one counts record per image, and
// histogram partials -> int64 histograms.  All sums are integers: any order is exact; the order here is fixed.
#include "cae_seg_metrics.hpp"

namespace cae {
namespace {

constexpr int kRecordThreads = 256;
constexpr int kSumThreads = 512;  // seg_histsum_kernel: 64 lanes x 4 words, 8 waves that share the partials out

// one block per image: the bx partials summed, the record written
__global__ __launch_bounds__(kRecordThreads) void seg_record_kernel(const unsigned long long *partial, int bx, int c,
                                                                    long long total, long long *counts) {
    const int n = blockIdx.x, tid = threadIdx.x;
    Tally<unsigned long long> ty = {{0, 0, 0, 0}};
    for (int b = tid; b < bx; b += kRecordThreads) {
#pragma unroll
        for (int j = 0; j < kPartial; ++j) ty.v[j] += partial[((size_t)n * bx + b) * kPartial + j];
    }
    const unsigned long long s = block_tally_sum<kRecordThreads>(ty);  // tally `tid` in the first lanes
    long long v[kPartial];
#pragma unroll
    for (int j = 0; j < kPartial; ++j) v[j] = (long long)__shfl(s, j, 64);
    if (tid == 0) {
        long long *out = counts + (size_t)n * 6;  // tp tn fp fn p tp_top
        if (c == 1) {
            out[0] = v[0], out[1] = v[1], out[2] = v[2], out[3] = v[3], out[4] = v[0] + v[3], out[5] = v[0];
        } else {
            const long long all = total < 0 ? v[2] : total, wrong = all - v[0];
            out[0] = v[0], out[1] = 0, out[2] = wrong, out[3] = wrong, out[4] = all, out[5] = v[1];
        }
    }
}

// hist[m][e] = the sum over the `sources` partials of output m of word e, e in 0 .. 2B: a block owns 256 words (four per
// lane), its waves take the partials in turn, and the eight wave sums are added in wave order
template <typename W>
__global__ __launch_bounds__(kSumThreads) void seg_histsum_kernel(const W *partial, int sources, uint32_t words,
                                                                  long long *out) {
    constexpr int kWaves = kSumThreads / 64;
    const uint32_t per_m = words / 256, m = blockIdx.x / per_m, first = (blockIdx.x % per_m) * 256u;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t e = first + 4u * lane;  // < words: words is a multiple of 256
    const W *src = partial + (size_t)m * sources * words + e;
    unsigned long long s[4] = {0, 0, 0, 0};
#pragma unroll 4
    for (int b = wave; b < sources; b += kWaves) {
        const W *q = src + (size_t)b * words;
        if constexpr (sizeof(W) == 4) {
            const uint4 v = *reinterpret_cast<const uint4 *>(q);
            s[0] += v.x, s[1] += v.y, s[2] += v.z, s[3] += v.w;
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) s[j] += q[j];
        }
    }
    __shared__ unsigned long long wave_sum[kWaves][256];
#pragma unroll
    for (int j = 0; j < 4; ++j) wave_sum[wave][4 * lane + j] = s[j];
    __syncthreads();
    if (threadIdx.x < 256) {
        unsigned long long t = 0;
#pragma unroll
        for (int k = 0; k < kWaves; ++k) t += wave_sum[k][threadIdx.x];
        out[(size_t)m * words + first + threadIdx.x] = (long long)t;
    }
}

}  // namespace

int launch_seg_record(const unsigned long long *partial, int n, int bx, int c, long long total, long long *counts,
                      hipStream_t st) {
    hipLaunchKernelGGL(seg_record_kernel, dim3(n), dim3(kRecordThreads), 0, st, partial, bx, c, total, counts);
    HIP_TRY(hipGetLastError());
    return CAE_OK;
}

template <typename W>
int launch_seg_histsum(const W *partial, int n, int bx, int per_image, int bits, long long *hist, hipStream_t st) {
    const uint32_t words = 2u << bits;
    const int m = per_image ? n : 1, sources = per_image ? bx : n * bx;
    hipLaunchKernelGGL(seg_histsum_kernel<W>, dim3((unsigned)((size_t)m * (words / 256))), dim3(kSumThreads), 0, st,
                       partial, sources, words, hist);
    HIP_TRY(hipGetLastError());
    return CAE_OK;
}
template int launch_seg_histsum(const uint32_t *, int, int, int, int, long long *, hipStream_t);
template int launch_seg_histsum(const unsigned long long *, int, int, int, int, long long *, hipStream_t);

}  // namespace cae
