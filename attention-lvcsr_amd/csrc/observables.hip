// Training and validation observables of the reference's train() (lvsr/main.py:317-396, 526-569; lvsr/expressions.py:14-25) as
// reductions on the device: the alignment penalty and entropy, min / max / mean |x| of a tensor, per-parameter norms of a step.
// They run behind the backward pass inside the step's graph region; the host copies a record of a few dozen numbers.
// lvsr_utterance_stats is the decode report's share (lvsr/main.py:732-736, 778-790, 816-823): cost, alignment spread and penalty per utterance.
// lvsr_alignment_times turns every label's alignment row into positions (peak, mean, quantiles of the running sum): what the reference
// shows as a picture (show_alignment, lvsr/notebook.py:81, lvsr/main.py:834-840) as numbers a caller can turn into seconds.
//
// Determinism: no floating-point atomics.  Every kernel pair is "fixed slices -> partials, one work-group adds the partials": the
// slices and the trees depend on the sizes alone, so eager launches, captured launches and graph replays give the same bits.
// Precision: a row's quantity is float32 where the reference's is; everything summed across rows, work-groups or tensors is float64.
//
// lvsr_segment_norms is TWO launches around lvsr_opt_step (phase 1 in front: parameter and gradient; phase 2 behind: step, sums):
// the reference monitors the parameter the gradient was taken at, and the optimiser overwrites it.
#include "common.h"
#include "lvsr_hip.h"
#include <limits.h>
#include <math.h>
#include <string.h>

#define OBS_THREADS 256
#define OBS_TS_CHUNK 8192               // elements of a tensor per work-group, until OBS_TS_MAX_PARTS work-groups are reached
#define OBS_TS_MAX_PARTS 1024
#define OBS_ITEM_MAX 8192               // elements of a work item of lvsr_segment_norms

// sum over the work-group's OBS_THREADS threads of K values each: a fixed binary tree through LDS; the totals end in red[k][0]
template <int K, int N>
__device__ __forceinline__ void obs_block_sum(const double* v, double (*red)[N]) {
    const int t = threadIdx.x;
#pragma unroll
    for (int k = 0; k < K; ++k) red[k][t] = v[k];
    __syncthreads();
    for (int s = N / 2; s > 0; s >>= 1) {
        if (t < s)
#pragma unroll
            for (int k = 0; k < K; ++k) red[k][t] += red[k][t + s];
        __syncthreads();
    }
}

// ---- alignment ------------------------------------------------------------------------------------------------------------------
// inclusive prefix sum over the 64 lanes (lane i: v_0 + ... + v_i; six rounded additions deep), as the column scan of reward.hip
__device__ __forceinline__ float obs_wave_scan(float v, int lane) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const float u = __shfl_up(v, o, 64);
        if (lane >= o) v += u;
    }
    return v;
}
// the value of lane 63 in every lane (an exact sum: the other lanes add zeros)
__device__ __forceinline__ float obs_last_lane(float v, int lane) { return wave_sum(lane == 63 ? v : 0.f); }

// one wave per row (l,b): partials[2 row] = mask * sum_t max(C[l,b,t] - C[l-1,b,t], 0) (l = 0: 0), [2 row + 1] = mask * sum_t w logf(w + 1e-7f)
__global__ __launch_bounds__(OBS_THREADS) void obs_align_rows_kernel(const float* w, long long ldw, int rows, int B, int Tp, const float* mask,
                                                                     double* partials) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= rows) return;
    const float* cur = w + (size_t)row * ldw;
    const float* prev = row >= B ? cur - (size_t)B * ldw : nullptr;
    float carry1 = 0.f, carry0 = 0.f, pen = 0.f, ent = 0.f;
    for (int c0 = 0; c0 < Tp; c0 += 64) {
        const int t = c0 + lane;
        const float a = t < Tp ? cur[t] : 0.f;
        ent += a * logf(a + 1e-7f);                        // a = 0: 0 * logf(1e-7f) = -0
        if (prev) {                                        // (uniform over the wave)
            const float p = t < Tp ? prev[t] : 0.f;
            const float s1 = obs_wave_scan(a, lane) + carry1, s0 = obs_wave_scan(p, lane) + carry0;
            if (t < Tp) pen += fmaxf(s1 - s0, 0.f);
            carry1 = obs_last_lane(s1, lane);
            carry0 = obs_last_lane(s0, lane);
        }
    }
    pen = wave_sum(pen);
    ent = wave_sum(ent);
    if (lane == 0) {
        const float m = mask ? mask[row] : 1.f;
        partials[2 * (size_t)row] = (double)(pen * m);
        partials[2 * (size_t)row + 1] = (double)(ent * m);
    }
}

__global__ __launch_bounds__(OBS_THREADS) void obs_align_sum_kernel(const double* partials, const float* mask, int rows, double* out,
                                                                    int accumulate) {
    __shared__ double red[3][OBS_THREADS];
    double s[3] = {0.0, 0.0, 0.0};
    for (int r = threadIdx.x; r < rows; r += OBS_THREADS) {
        s[0] += partials[2 * (size_t)r];
        s[1] += partials[2 * (size_t)r + 1];
        s[2] += mask ? (double)mask[r] : 1.0;
    }
    obs_block_sum<3>(s, red);
    if (threadIdx.x < 3) out[threadIdx.x] = (accumulate ? out[threadIdx.x] : 0.0) + red[threadIdx.x][0];
}

// ---- per-utterance alignment and cost (the decode report) ---------------------------------------------------------------------
__device__ __forceinline__ double obs_shfl_xor_f64(double v, int o) {
    int h[2];
    memcpy(h, &v, sizeof(v));
    h[0] = __shfl_xor(h[0], o, 64);
    h[1] = __shfl_xor(h[1], o, 64);
    memcpy(&v, h, sizeof(v));
    return v;
}
__device__ __forceinline__ double obs_wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += obs_shfl_xor_f64(v, o);
    return v;
}

// one wave per row (l,b), over the utterance's own attended length n = lengths[b] (NULL: T'): partials[3 row] = m cost,
// [3 row + 1] = m sqrt(max(E2 - E1^2, 0)) with the moments in float64, [3 row + 2] = m sum_{t<n} max(C[l,b,t] - C[l-1,b,t], 0) with
// the float32 scan of obs_align_rows_kernel (l = 0: 0).  A row whose mask is 0 writes zeros and reads neither weights nor costs.
__global__ __launch_bounds__(OBS_THREADS) void obs_utt_rows_kernel(const float* w, long long ldw, int rows, int B, int Tp, const float* mask,
                                                                   const float* costs, const int* lengths, double* partials) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= rows) return;
    double* out = partials + 3 * (size_t)row;
    const float m = mask ? mask[row] : 1.f;
    if (m == 0.f) {                                        // (uniform over the wave)
        if (lane < 3) out[lane] = 0.0;
        return;
    }
    int n = lengths ? lengths[row % B] : Tp;
    n = n < 0 ? 0 : n > Tp ? Tp : n;
    const float* cur = w + (size_t)row * ldw;
    const float* prev = row >= B ? cur - (size_t)B * ldw : nullptr;
    float carry1 = 0.f, carry0 = 0.f, pen = 0.f;
    double e1 = 0.0, e2 = 0.0;
    for (int c0 = 0; c0 < n; c0 += 64) {
        const int t = c0 + lane;
        const float a = t < n ? cur[t] : 0.f;
        const double at = (double)a * (double)t;           // exact while t < 2^29
        e1 += at;
        e2 += at * (double)t;
        if (prev) {                                        // (uniform over the wave)
            const float p = t < n ? prev[t] : 0.f;
            const float s1 = obs_wave_scan(a, lane) + carry1, s0 = obs_wave_scan(p, lane) + carry0;
            if (t < n) pen += fmaxf(s1 - s0, 0.f);
            carry1 = obs_last_lane(s1, lane);
            carry0 = obs_last_lane(s0, lane);
        }
    }
    pen = wave_sum(pen);
    e1 = obs_wave_sum_f64(e1);
    e2 = obs_wave_sum_f64(e2);
    if (lane == 0) {
        const double md = (double)m;
        out[0] = costs ? md * (double)costs[row] : 0.0;
        out[1] = md * sqrt(fmax(e2 - e1 * e1, 0.0));
        out[2] = md * (double)pen;
    }
}

// one wave per utterance b: out[b] = (sum_l partials[3 (l B + b) + k], k < 3; sum_l mask[l,b]), lanes strided over the labels, then
// the xor tree, all in float64
__global__ __launch_bounds__(64) void obs_utt_sum_kernel(const double* partials, const float* mask, int L, int B, double* out) {
    const int b = blockIdx.x, lane = threadIdx.x;
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    for (int l = lane; l < L; l += 64) {
        const size_t row = (size_t)l * B + b;
#pragma unroll
        for (int k = 0; k < 3; ++k) s[k] += partials[3 * row + k];
        s[3] += mask ? (double)mask[row] : 1.0;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) s[k] = obs_wave_sum_f64(s[k]);
    if (lane == 0)
#pragma unroll
        for (int k = 0; k < 4; ++k) out[4 * (size_t)b + k] = s[k];
}

// ---- per-label alignment times (recognising with time stamps) -------------------------------------------------------------------
// the smallest index over the wave (lanes that found none hold INT_MAX)
__device__ __forceinline__ int obs_wave_min_int(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
    return v;
}

// one wave per row (l,b), over n = lengths[b] (NULL: T') positions: out[8 row + k] = peak, w[peak], E1, sqrt(max(E2 - E1^2, 0)),
// start, end, C[n-1], cost (include/lvsr_hip.h).  Two walks over the row with the same float32 scan (so the same bits): the first
// finds the peak, the moments and C[n-1], the second the first positions at which C reaches lo C[n-1] and hi C[n-1].  A row whose
// mask is 0 or whose n is 0 writes eight zeros and reads neither weights nor costs.
__global__ __launch_bounds__(OBS_THREADS) void obs_align_times_kernel(const float* w, long long ldw, int rows, int B, int Tp, const float* mask,
                                                                      const float* costs, const int* lengths, float lo, float hi, double* out8) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= rows) return;
    double* out = out8 + 8 * (size_t)row;
    const float m = mask ? mask[row] : 1.f;
    int n = lengths ? lengths[row % B] : Tp;
    n = n < 0 ? 0 : n > Tp ? Tp : n;
    if (m == 0.f || n == 0) {                              // (uniform over the wave)
        if (lane < 8) out[lane] = 0.0;
        return;
    }
    const float* cur = w + (size_t)row * ldw;
    float carry = 0.f, best = -INFINITY;
    int peak = INT_MAX;
    double e1 = 0.0, e2 = 0.0;
    for (int c0 = 0; c0 < n; c0 += 64) {
        const int t = c0 + lane;
        const float a = t < n ? cur[t] : 0.f;
        const double at = (double)a * (double)t;           // exact while t < 2^29
        e1 += at;
        e2 += at * (double)t;
        if (t < n && a > best) {                           // a lane meets its positions in rising order: `>` keeps the first
            best = a;
            peak = t;
        }
        carry = obs_last_lane(obs_wave_scan(a, lane) + carry, lane);       // lanes behind n add zeros: the last carry is C[n-1]
    }
    // (value, index) pairs through the xor tree: the larger value, on equal values the smaller index
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(best, o, 64);
        const int oi = __shfl_xor(peak, o, 64);
        if (ov > best || (ov == best && oi < peak)) {
            best = ov;
            peak = oi;
        }
    }
    e1 = obs_wave_sum_f64(e1);
    e2 = obs_wave_sum_f64(e2);
    const float total = carry, thr_lo = lo * total, thr_hi = hi * total;
    int start = INT_MAX, end = INT_MAX;
    carry = 0.f;
    for (int c0 = 0; c0 < n; c0 += 64) {
        const int t = c0 + lane;
        const float s = obs_wave_scan(t < n ? cur[t] : 0.f, lane) + carry;
        if (t < n && s >= thr_lo) start = min(start, t);
        if (t < n && s >= thr_hi) end = min(end, t);
        carry = obs_last_lane(s, lane);
    }
    start = obs_wave_min_int(start);
    end = obs_wave_min_int(end);
    if (lane == 0) {
        // 0 <= lo, hi <= 1 and weights >= 0: C[n-1] itself reaches both thresholds.  Anything else (a NaN, negative weights) still
        // gives positions inside the row.
        out[0] = (double)(peak < n ? peak : 0);
        out[1] = (double)best;
        out[2] = e1;
        out[3] = sqrt(fmax(e2 - e1 * e1, 0.0));
        out[4] = (double)(start < n ? start : n - 1);
        out[5] = (double)(end < n ? end : n - 1);
        out[6] = (double)total;
        out[7] = costs ? (double)costs[row] : 0.0;
    }
}

// ---- min, max, sum |x| ----------------------------------------------------------------------------------------------------------
// v = (min, max, sum): the tree of obs_block_sum with the three operations
__device__ __forceinline__ void obs_block_mms(const double* v, double (*red)[OBS_THREADS]) {
    const int t = threadIdx.x;
    red[0][t] = v[0]; red[1][t] = v[1]; red[2][t] = v[2];
    __syncthreads();
    for (int s = OBS_THREADS / 2; s > 0; s >>= 1) {
        if (t < s) {
            red[0][t] = fmin(red[0][t], red[0][t + s]);
            red[1][t] = fmax(red[1][t], red[1][t + s]);
            red[2][t] += red[2][t + s];
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(OBS_THREADS) void obs_tstats_part_kernel(const float* x, long long n, int use_floor, float floor, double* partials) {
    __shared__ double red[3][OBS_THREADS];
    float mn = INFINITY, mx = -INFINITY;
    double sum = 0.0;
    for (long long i = (long long)blockIdx.x * OBS_THREADS + threadIdx.x; i < n; i += (long long)gridDim.x * OBS_THREADS) {
        float v = x[i];
        if (use_floor) v = fmaxf(v, floor);
        mn = fminf(mn, v);
        mx = fmaxf(mx, v);
        sum += (double)fabsf(v);
    }
    const double v[3] = {(double)mn, (double)mx, sum};
    obs_block_mms(v, red);
    if (threadIdx.x < 3) partials[3 * (size_t)blockIdx.x + threadIdx.x] = red[threadIdx.x][0];
}

__global__ __launch_bounds__(OBS_THREADS) void obs_tstats_sum_kernel(const double* partials, int nparts, double* out) {
    __shared__ double red[3][OBS_THREADS];
    double v[3] = {(double)INFINITY, -(double)INFINITY, 0.0};
    for (int b = threadIdx.x; b < nparts; b += OBS_THREADS) {
        v[0] = fmin(v[0], partials[3 * (size_t)b]);
        v[1] = fmax(v[1], partials[3 * (size_t)b + 1]);
        v[2] += partials[3 * (size_t)b + 2];
    }
    obs_block_mms(v, red);
    if (threadIdx.x < 3) out[threadIdx.x] = red[threadIdx.x][0];
}

// ---- per-parameter norms --------------------------------------------------------------------------------------------------------
typedef lvsr_segnorm_args SN;

// one work-group per item; what bit 0: sums of p^2 and (g grad_scale)^2 -> partials[3 item + 0, 1]; bit 1: of step^2 -> [3 item + 2]
__global__ __launch_bounds__(OBS_THREADS) void obs_segnorm_items_kernel(SN a, int what) {
    __shared__ double red[3][OBS_THREADS];
    const long long* it = a.items + 3 * (size_t)blockIdx.x;
    const long long seg = it[0], start = it[1], count = it[2];
    if (seg < 0 || seg >= a.nseg) return;                                   // (uniform: a malformed table reads nothing)
    const long long size = a.segments[4 * seg + 1] * a.segments[4 * seg + 2];
    if (start < 0 || count < 0 || count > OBS_ITEM_MAX || start + count > size) return;
    const long long off = a.segments[4 * seg] + start;
    double s[3] = {0.0, 0.0, 0.0};
    for (long long i = threadIdx.x; i < count; i += OBS_THREADS) {
        if (what & 1) {
            const double p = (double)a.param[off + i], g = (double)(a.grad[off + i] * a.grad_scale);
            s[0] += p * p;
            s[1] += g * g;
        }
        if (what & 2) {
            const double d = (double)a.step[off + i];
            s[2] += d * d;
        }
    }
    obs_block_sum<3>(s, red);
    const int k = threadIdx.x;
    if ((k < 2 && (what & 1)) || (k == 2 && (what & 2))) a.partials[3 * (size_t)blockIdx.x + k] = red[k][0];
}

// one work-group (one wave) per segment: its items' partials, lanes strided over the items, then the tree
__global__ __launch_bounds__(64) void obs_segnorm_final_kernel(SN a) {
    __shared__ double red[3][64];
    const int seg = blockIdx.x, lane = threadIdx.x;
    const int i0 = a.seg_first[seg], i1 = a.seg_first[seg + 1];
    if (i0 < 0 || i1 < i0 || i1 > a.nitems) return;
    double s[3] = {0.0, 0.0, 0.0};
    for (int it = i0 + lane; it < i1; it += 64)
#pragma unroll
        for (int k = 0; k < 3; ++k) s[k] += a.partials[3 * (size_t)it + k];
    obs_block_sum<3>(s, red);
    if (lane == 0) {
        const double sp = red[0][0], sg = red[1][0];
        double ss = red[2][0];
        // what the optimiser's last kernel did to `step` on the fly (opt_apply_kernel): guarded step, BurnIn, RemoveNotFinite
        const bool skipped = a.scratch && a.scratch[3] != 0.f;
        const bool burn = a.clip_state && a.scratch && a.scratch[2] != 0.f;
        if (skipped || burn) ss = 0.0;
        else if (a.remove_not_finite && a.segflag && a.segflag[seg]) {
            const double k = 1.0 - (double)a.nonfinite_scaler;
            ss = k * k * sp;
        }
        a.segsums[3 * (size_t)seg] = sp;
        a.segsums[3 * (size_t)seg + 1] = sg;
        a.segsums[3 * (size_t)seg + 2] = ss;
        const double root = sqrt((double)(a.segments[4 * (size_t)seg + 1] * a.segments[4 * (size_t)seg + 2]));
        float* o = a.out + 4 * (size_t)seg;
        o[0] = (float)(sqrt(sp) / root);
        o[1] = (float)(sqrt(sg) / root);
        o[2] = (float)(sqrt(ss) / root);
        o[3] = o[2] / o[1];
    }
}

__global__ __launch_bounds__(OBS_THREADS) void obs_segnorm_total_kernel(SN a) {
    __shared__ double red[1][OBS_THREADS];
    double s[1] = {0.0};
    for (int seg = threadIdx.x; seg < a.nseg; seg += OBS_THREADS) s[0] += a.segsums[3 * (size_t)seg + 2];
    obs_block_sum<1>(s, red);
    if (threadIdx.x == 0) a.total[0] = sqrt(red[0][0]);
}

extern "C" {

int lvsr_alignment_stats(void* stream, const float* weights, long long ldw, int L, int B, int Tp, const float* mask, double* partials,
                         double* out, int accumulate) {
    LVSR_REQUIRE(weights && partials && out, "lvsr_alignment_stats: null argument");
    LVSR_REQUIRE(L > 0 && B > 0 && Tp > 0 && ldw >= Tp, "lvsr_alignment_stats: bad sizes (L, B, T' > 0; ldw >= T')");
    LVSR_REQUIRE((long long)L * B <= (1ll << 30), "lvsr_alignment_stats: more than 2^30 rows");
    const int rows = L * B;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(obs_align_rows_kernel, dim3((rows + 3) / 4), dim3(OBS_THREADS), 0, s, weights, ldw, rows, B, Tp, mask, partials);
    hipLaunchKernelGGL(obs_align_sum_kernel, dim3(1), dim3(OBS_THREADS), 0, s, (const double*)partials, mask, rows, out, accumulate);
    return lvsr_check_launch("lvsr_alignment_stats");
}

int lvsr_utterance_stats(void* stream, const float* weights, long long ldw, int L, int B, int Tp, const float* mask, const float* costs,
                         const int* lengths, double* partials, double* out) {
    LVSR_REQUIRE(weights && partials && out, "lvsr_utterance_stats: null argument");
    LVSR_REQUIRE(L > 0 && B > 0 && Tp > 0 && ldw >= Tp, "lvsr_utterance_stats: bad sizes (L, B, T' > 0; ldw >= T')");
    LVSR_REQUIRE((long long)L * B <= (1ll << 30), "lvsr_utterance_stats: more than 2^30 rows");
    const int rows = L * B;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(obs_utt_rows_kernel, dim3((rows + 3) / 4), dim3(OBS_THREADS), 0, s, weights, ldw, rows, B, Tp, mask, costs, lengths,
                       partials);
    hipLaunchKernelGGL(obs_utt_sum_kernel, dim3(B), dim3(64), 0, s, (const double*)partials, mask, L, B, out);
    return lvsr_check_launch("lvsr_utterance_stats");
}

int lvsr_alignment_times(void* stream, const float* weights, long long ldw, int L, int B, int Tp, const float* mask, const float* costs,
                         const int* lengths, float lo, float hi, double* out) {
    LVSR_REQUIRE(weights && out, "lvsr_alignment_times: null argument");
    LVSR_REQUIRE(L > 0 && B > 0 && Tp > 0 && ldw >= Tp, "lvsr_alignment_times: bad sizes (L, B, T' > 0; ldw >= T')");
    LVSR_REQUIRE((long long)L * B <= (1ll << 30), "lvsr_alignment_times: more than 2^30 rows");
    LVSR_REQUIRE(0.f <= lo && lo <= hi && hi <= 1.f, "lvsr_alignment_times: quantiles must satisfy 0 <= lo <= hi <= 1");       // (a NaN fails)
    const int rows = L * B;
    hipLaunchKernelGGL(obs_align_times_kernel, dim3((rows + 3) / 4), dim3(OBS_THREADS), 0, (hipStream_t)stream, weights, ldw, rows, B, Tp,
                       mask, costs, lengths, lo, hi, out);
    return lvsr_check_launch("lvsr_alignment_times");
}

int lvsr_tensor_stats(void* stream, const float* x, long long n, int use_floor, float floor, double* partials, double* out) {
    LVSR_REQUIRE(x && partials && out, "lvsr_tensor_stats: null argument");
    LVSR_REQUIRE(n > 0, "lvsr_tensor_stats: an empty tensor has no minimum");
    long long parts = (n + OBS_TS_CHUNK - 1) / OBS_TS_CHUNK;
    if (parts > OBS_TS_MAX_PARTS) parts = OBS_TS_MAX_PARTS;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(obs_tstats_part_kernel, dim3((unsigned)parts), dim3(OBS_THREADS), 0, s, x, n, use_floor, floor, partials);
    hipLaunchKernelGGL(obs_tstats_sum_kernel, dim3(1), dim3(OBS_THREADS), 0, s, (const double*)partials, (int)parts, out);
    return lvsr_check_launch("lvsr_tensor_stats");
}

int lvsr_segment_norms(void* stream, const lvsr_segnorm_args* args, int phase) {
    LVSR_REQUIRE(args != nullptr, "lvsr_segment_norms: null args");
    LVSR_REQUIRE(phase >= 1 && phase <= 3, "lvsr_segment_norms: phase is 1 (in front of the optimiser), 2 (behind it) or 3 (both)");
    SN a;
    memcpy(&a, args, sizeof(a));
    LVSR_REQUIRE(a.nseg > 0 && a.nitems > 0 && a.segments && a.items && a.seg_first && a.partials, "lvsr_segment_norms: missing tables");
    LVSR_REQUIRE(!(phase & 1) || (a.param && a.grad), "lvsr_segment_norms: phase 1 reads param and grad");
    LVSR_REQUIRE(!(phase & 2) || (a.step && a.segsums && a.out && a.total), "lvsr_segment_norms: phase 2 reads step and writes segsums, out, total");
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(obs_segnorm_items_kernel, dim3(a.nitems), dim3(OBS_THREADS), 0, s, a, phase);
    if (phase & 2) {
        hipLaunchKernelGGL(obs_segnorm_final_kernel, dim3(a.nseg), dim3(64), 0, s, a);
        hipLaunchKernelGGL(obs_segnorm_total_kernel, dim3(1), dim3(OBS_THREADS), 0, s, a);
    }
    return lvsr_check_launch("lvsr_segment_norms");
}

}  // extern "C"
