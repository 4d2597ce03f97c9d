// Adaptive weight noise (Graves, NIPS 2011): the reference's apply_adaptive_noise (lvsr/graph.py:71-249, wired at
// lvsr/main.py:425-456) as two passes over the flat parameter layout per training step:
//   head  lvsr_wnoise_sample: noisy weights mu + z sqrt(s2) into the store's buffer, float64 sums of mu, mu^2, s2, ls2 (fixed
//         order), then one work-group forms prior_u, prior_s2 and the model cost (as opt_norm_kernel follows opt_sqnorm_kernel);
//   tail  lvsr_wnoise_grad: the gradient rewrite [d/dmu | d/dls2] behind the (all-reduced) task gradient, and the step counter.
// The noise is a counter-based Philox4x32-10 stream (not Theano's MRG31k3p): element i of step c is a pure function of
// (seed, c, i), so graph replays, ranks and the emulator draw the same numbers (include/lvsr_hip.h).
#include "common.h"
#include "lvsr_hip.h"
#include <string.h>

typedef lvsr_wnoise_args WN;

#define WN_SCALE 2048.f                 // log_sigma_scale, lvsr/graph.py:159
#define WN_THREADS 256
#define WN_MAX_PARTS 1024               // 256 CUs x 4 work-groups of 256 threads: one resident wave of work-groups
#define WN_STATS 8

__device__ __forceinline__ void philox4x32_10(unsigned c[4], unsigned k0, unsigned k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned long long p0 = (unsigned long long)0xD2511F53u * c[0];
        const unsigned long long p1 = (unsigned long long)0xCD9E8D57u * c[2];
        const unsigned n0 = (unsigned)(p1 >> 32) ^ c[1] ^ k0, n1 = (unsigned)p1;
        const unsigned n2 = (unsigned)(p0 >> 32) ^ c[3] ^ k1, n3 = (unsigned)p0;
        c[0] = n0; c[1] = n1; c[2] = n2; c[3] = n3;
        k0 += 0x9E3779B9u;              // (the bump after the tenth round is never used)
        k1 += 0xBB67AE85u;
    }
}

// the four normals of Philox block q (elements 4q .. 4q+3) of step `step`
__device__ __forceinline__ void philox_normal4(unsigned long long key, unsigned long long q, unsigned long long step, float z[4],
                                               unsigned* raw) {
    unsigned c[4] = {(unsigned)q, (unsigned)(q >> 32), (unsigned)step, (unsigned)(step >> 32)};
    philox4x32_10(c, (unsigned)key, (unsigned)(key >> 32));
    if (raw) {
        raw[0] = c[0]; raw[1] = c[1]; raw[2] = c[2]; raw[3] = c[3];
    }
    float u[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) u[j] = (float)(2u * (c[j] >> 9) + 1u) * 5.9604644775390625e-8f;     // (2k+1) 2^-24: in (0,1), exact
#pragma unroll
    for (int j = 0; j < 4; j += 2) {
        const float r = sqrtf(-2.f * logf(u[j]));
        const float t = 6.28318530717958647692f * u[j + 1];
        z[j] = r * cosf(t);
        z[j + 1] = r * sinf(t);
    }
}

// first Philox block >= c0 of the grid-stride sequence of global work-item `gid` (stride `stride`): every segment is walked with the
// same global partition of the block index space, so the work spreads over the whole grid whatever the segment sizes
__device__ __forceinline__ long long wn_first(long long c0, long long gid, long long stride) {
    const long long r = c0 % stride;
    return c0 + (gid >= r ? gid - r : gid - r + stride);
}

__device__ __forceinline__ void wn_block_sum4(double v[4], double (*red)[WN_THREADS]) {
    const int t = threadIdx.x;
#pragma unroll
    for (int k = 0; k < 4; ++k) red[k][t] = v[k];
    __syncthreads();
    for (int s = WN_THREADS / 2; s > 0; s >>= 1) {
        if (t < s)
#pragma unroll
            for (int k = 0; k < 4; ++k) red[k][t] += red[k][t + s];
        __syncthreads();
    }
}

__global__ __launch_bounds__(WN_THREADS) void wnoise_sample_kernel(WN a) {
    __shared__ double red[4][WN_THREADS];
    const unsigned long long key = (unsigned long long)a.seed, step = (unsigned long long)a.counter[0];
    const long long stride = (long long)gridDim.x * WN_THREADS, gid = (long long)blockIdx.x * WN_THREADS + threadIdx.x;
    double sum[4] = {0.0, 0.0, 0.0, 0.0};            // mu, mu^2, s2, ls2
    for (int sg = 0; sg < a.nseg; ++sg) {
        const long long off = a.segments[4 * sg], cnt = a.segments[4 * sg + 1] * a.segments[4 * sg + 2];
        const long long c0 = off >> 2, c1 = c0 + ((cnt + 3) >> 2);
        for (long long q = wn_first(c0, gid, stride); q < c1; q += stride) {
            float z[4];
            philox_normal4(key, (unsigned long long)q, step, z, nullptr);
            const long long i = q << 2, rem = off + cnt - i;
            float m[4], l[4], s2[4], w[4];
            if (rem >= 4) {
                const float4 mv = *(const float4*)(a.mu + i), lv = *(const float4*)(a.ls2 + i);
                m[0] = mv.x; m[1] = mv.y; m[2] = mv.z; m[3] = mv.w;
                l[0] = lv.x; l[1] = lv.y; l[2] = lv.z; l[3] = lv.w;
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    m[j] = j < rem ? a.mu[i + j] : 0.f;
                    l[j] = j < rem ? a.ls2[i + j] : 0.f;
                }
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                s2[j] = expf(l[j] * WN_SCALE);                       // p_s2 = exp(p_ls2 * log_sigma_scale), graph.py:178
                w[j] = m[j] + z[j] * sqrtf(s2[j]);                   // graph.py:181
            }
            if (rem >= 4) {
                *(float4*)(a.noisy + i) = make_float4(w[0], w[1], w[2], w[3]);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    sum[0] += (double)m[j];
                    sum[1] += (double)m[j] * (double)m[j];
                    sum[2] += (double)s2[j];
                    sum[3] += (double)l[j];
                }
            } else {
                for (int j = 0; j < rem; ++j) {
                    a.noisy[i + j] = w[j];
                    sum[0] += (double)m[j];
                    sum[1] += (double)m[j] * (double)m[j];
                    sum[2] += (double)s2[j];
                    sum[3] += (double)l[j];
                }
            }
        }
    }
    wn_block_sum4(sum, red);
    if (threadIdx.x < 4) a.stats[WN_STATS + 4 * blockIdx.x + threadIdx.x] = red[threadIdx.x][0];
}

// one work-group: the partials in a fixed order -> prior_u, prior_s2 (float32, graph.py:185-197) and the model cost (:205-212)
__global__ __launch_bounds__(WN_THREADS) void wnoise_prior_kernel(WN a, int nparts) {
    __shared__ double red[4][WN_THREADS];
    double sum[4] = {0.0, 0.0, 0.0, 0.0};
    for (int b = threadIdx.x; b < nparts; b += WN_THREADS)
#pragma unroll
        for (int k = 0; k < 4; ++k) sum[k] += a.stats[WN_STATS + 4 * b + k];
    wn_block_sum4(sum, red);
    if (threadIdx.x == 0) {
        double count = 0.0;
        for (int sg = 0; sg < a.nseg; ++sg) count += (double)(a.segments[4 * sg + 1] * a.segments[4 * sg + 2]);
        const double su = red[0][0], su2 = red[1][0], ss2 = red[2][0], sls = red[3][0];
        const float pu = (float)(su / count);
        const double u = (double)pu;
        const double dev = su2 - 2.0 * u * su + count * u * u;       // sum (mu - prior_u)^2
        const float ps2 = (float)((ss2 + dev) / count);
        const double p = (double)ps2;
        const double lc = (0.5 * (count * log(p) - (double)WN_SCALE * sls) + (dev + ss2 - count * p) / (2.0 * p))
                          / a.num_examples * a.coef;
        a.stats[0] = su; a.stats[1] = su2; a.stats[2] = ss2; a.stats[3] = sls;
        a.stats[4] = u; a.stats[5] = p; a.stats[6] = lc; a.stats[7] = count;
    }
}

__global__ __launch_bounds__(WN_THREADS) void wnoise_grad_kernel(WN a) {
    const float pu = (float)a.stats[4], ps2 = (float)a.stats[5];
    const float nps2 = (float)a.num_examples * ps2, coef = (float)a.coef;
    const double kls = a.coef * 0.5 / a.num_examples * (double)WN_SCALE;
    const float hs = 0.5f * WN_SCALE;
    const long long stride = (long long)gridDim.x * WN_THREADS, gid = (long long)blockIdx.x * WN_THREADS + threadIdx.x;
    for (int sg = 0; sg < a.nseg; ++sg) {
        const long long off = a.segments[4 * sg], cnt = a.segments[4 * sg + 1] * a.segments[4 * sg + 2];
        const long long c0 = off >> 2, c1 = c0 + ((cnt + 3) >> 2);
        for (long long q = wn_first(c0, gid, stride); q < c1; q += stride) {
            const long long i = q << 2, rem = off + cnt - i;
            float m[4], l[4], g[4], dm[4], dl[4];
            if (rem >= 4) {
                const float4 mv = *(const float4*)(a.mu + i), lv = *(const float4*)(a.ls2 + i), gv = *(const float4*)(a.grad + i);
                m[0] = mv.x; m[1] = mv.y; m[2] = mv.z; m[3] = mv.w;
                l[0] = lv.x; l[1] = lv.y; l[2] = lv.z; l[3] = lv.w;
                g[0] = gv.x; g[1] = gv.y; g[2] = gv.z; g[3] = gv.w;
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    m[j] = j < rem ? a.mu[i + j] : 0.f;
                    l[j] = j < rem ? a.ls2[i + j] : 0.f;
                    g[j] = j < rem ? a.grad[i + j] : 0.f;
                }
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float gg = g[j] * a.grad_scale;
                const float s2 = expf(l[j] * WN_SCALE);
                dm[j] = coef * (m[j] - pu) / nps2 + gg;                        // graph.py:240-241
                // :243-247; the two terms cancel where the model cost and the Hessian estimate balance: summed in float64
                const double gd = (double)g[j] * (double)a.grad_scale;
                dl[j] = (float)(kls * ((double)s2 / (double)ps2 - 1.0) + (double)hs * (double)s2 * (gd * gd));
                if (j >= rem) dm[j] = dl[j] = 0.f;                               // padding
            }
            *(float4*)(a.gtheta + i) = make_float4(dm[0], dm[1], dm[2], dm[3]);
            *(float4*)(a.gtheta + a.n + i) = make_float4(dl[0], dl[1], dl[2], dl[3]);
        }
    }
    // the sampler of this step (the only reader of the counter) finished earlier on this stream
    if (blockIdx.x == 0 && threadIdx.x == 0) a.counter[0] = a.counter[0] + 1;
}

__global__ __launch_bounds__(WN_THREADS) void philox_normal_kernel(unsigned long long key, unsigned long long step,
                                                                   unsigned long long first, long long nblocks, float* z,
                                                                   unsigned* raw) {
    const long long b = (long long)blockIdx.x * WN_THREADS + threadIdx.x;
    if (b >= nblocks) return;
    float v[4];
    philox_normal4(key, first + (unsigned long long)b, step, v, raw ? raw + 4 * b : nullptr);
    *(float4*)(z + 4 * b) = make_float4(v[0], v[1], v[2], v[3]);
}

static int wn_parts(long long n) {
    const long long blocks = (n / 4 + 4 * WN_THREADS - 1) / (4 * WN_THREADS);      // >= 4 Philox blocks per work-item before the cap
    return (int)(blocks < 1 ? 1 : blocks > WN_MAX_PARTS ? WN_MAX_PARTS : blocks);
}

static int wn_check(const WN& a, const char* what) {
    LVSR_REQUIRE(a.n > 0 && (a.n & 3) == 0 && a.nseg > 0 && a.segments && a.mu && a.ls2 && a.counter && a.stats, "%s: missing buffers",
                 what);
    LVSR_REQUIRE(a.num_examples > 0.0, "%s: num_examples must be positive", what);
    return 0;
}

extern "C" int lvsr_wnoise_sample(void* stream, const lvsr_wnoise_args* args) {
    LVSR_REQUIRE(args != nullptr, "lvsr_wnoise_sample: null args");
    WN a;
    memcpy(&a, args, sizeof(a));
    if (wn_check(a, "lvsr_wnoise_sample")) return -1;
    LVSR_REQUIRE(a.noisy, "lvsr_wnoise_sample: missing the output buffer");
    const int nparts = wn_parts(a.n);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(wnoise_sample_kernel, dim3(nparts), dim3(WN_THREADS), 0, s, a);
    hipLaunchKernelGGL(wnoise_prior_kernel, dim3(1), dim3(WN_THREADS), 0, s, a, nparts);
    return lvsr_check_launch("lvsr_wnoise_sample");
}

extern "C" int lvsr_wnoise_grad(void* stream, const lvsr_wnoise_args* args) {
    LVSR_REQUIRE(args != nullptr, "lvsr_wnoise_grad: null args");
    WN a;
    memcpy(&a, args, sizeof(a));
    if (wn_check(a, "lvsr_wnoise_grad")) return -1;
    LVSR_REQUIRE(a.grad && a.gtheta, "lvsr_wnoise_grad: missing the gradient buffers");
    hipLaunchKernelGGL(wnoise_grad_kernel, dim3(wn_parts(a.n)), dim3(WN_THREADS), 0, (hipStream_t)stream, a);
    return lvsr_check_launch("lvsr_wnoise_grad");
}

extern "C" int lvsr_philox_normal(void* stream, long long seed, long long counter, long long first, long long nblocks, float* z,
                                  unsigned* raw) {
    LVSR_REQUIRE(nblocks >= 0 && (nblocks == 0 || z), "lvsr_philox_normal: bad arguments");
    if (nblocks == 0) return 0;
    const long long grid = (nblocks + WN_THREADS - 1) / WN_THREADS;
    LVSR_REQUIRE(grid < (1ll << 31), "lvsr_philox_normal: too many blocks");
    hipLaunchKernelGGL(philox_normal_kernel, dim3((unsigned)grid), dim3(WN_THREADS), 0, (hipStream_t)stream,
                       (unsigned long long)seed, (unsigned long long)counter, (unsigned long long)first, nblocks, z, raw);
    return lvsr_check_launch("lvsr_philox_normal");
}
