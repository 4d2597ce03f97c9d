// Task-loss-estimation criteria (mse_gain / mse_reward): the reward and gain matrices of a prediction against its
// groundtruth, and the regression cost of the readouts on them with its gradient.
//
// Reference semantics: RewardOp.perform (lvsr/ops.py:236-294) on reward_matrix / gain_matrix (lvsr/error_rate.py:79-112), which
// the reference evaluates in host Python per minibatch; RewardRegressionEmitter.cost (lvsr/bricks/__init__.py:134-183) with the
// mask of BaseSequenceGenerator.cost_matrix (libs/blocks/blocks/bricks/sequence_generators.py:317-326); the prediction mask of
// lvsr/main.py:254-259.  Here the edit-distance programme runs on the device, so that a training step stays one graph.
#include "common.h"
#include "lvsr_hip.h"

#define RG_MAX_Y 1024          // groundtruth positions (incl. its EOS) an utterance may have
#define RG_MAX_V 2048          // characters (lvsr_readout_step's limit)
#define RG_BIG (1 << 28)
#define RM_MAX_L 4096          // label positions of the mse_reward prefix / suffix sums

// One wave per utterance; the columns of the edit-distance table (one per prediction position) follow each other, the rows of
// a column are spread over the lanes in chunks of 64.  col_j[i] = edit distance between y[:i] and yhat[:j], i = 0..ny:
//   t[i] = min(col_{j-1}[i] + 1, col_{j-1}[i-1] + (y[i-1] != yhat[j-1])),  t[0] = j
//   col_j[i] = min(t[i], col_j[i-1] + 1)   <=>   col_j[i] - i = prefix_min_{k <= i} (t[k] - k)
// All integer: the per-character minimum below is an order-independent LDS atomic, the results are the same bits in any run.
__global__ __launch_bounds__(64) void reward_gain_kernel(const long long* gt, int Lg, const long long* pred, int Lp, int B,
                                                         long long eos, int V, float* rewards, float* gains, float* pmask) {
    __shared__ long long y[RG_MAX_Y];
    __shared__ int col[2][RG_MAX_Y + 1];
    __shared__ int best[RG_MAX_V];
    __shared__ int first[2];
    const int b = blockIdx.x, lane = threadIdx.x;
    if (lane < 2) first[lane] = lane == 0 ? Lg - 1 : Lp - 1;
    __syncthreads();
    // ny = groundtruth length up to and including its first EOS (none: the whole column); n = the same for the prediction
    for (int i = lane; i < Lg; i += 64) {
        const long long c = gt[(size_t)i * B + b];
        y[i] = c;
        if (c == eos) atomicMin(&first[0], i);
    }
    for (int j = lane; j < Lp; j += 64)
        if (pred[(size_t)j * B + b] == eos) atomicMin(&first[1], j);
    __syncthreads();
    const int ny = first[0] + 1, n = first[1] + 1;
    int prev_pick = 0;                                   // reward[j-1, yhat[j-1]]
    for (int j = 0; j < n; ++j) {
        int* cur = col[j & 1];
        const int* old = col[(j & 1) ^ 1];
        const long long ph = j > 0 ? pred[(size_t)(j - 1) * B + b] : 0;
        int carry = RG_BIG, cmin = RG_BIG;
        for (int c0 = 0; c0 <= ny; c0 += 64) {
            const int i = c0 + lane;
            int v = RG_BIG;
            if (i <= ny) {
                int t;
                if (j == 0) t = i;
                else if (i == 0) t = j;
                else t = min(old[i] + 1, old[i - 1] + (y[i - 1] != ph ? 1 : 0));
                v = t - i;
            }
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const int u = __shfl_up(v, o, 64);
                if (lane >= o) v = min(v, u);
            }
            v = min(v, carry);
            int m = RG_BIG;
            if (i <= ny) { cur[i] = v + i; m = v + i; }
            int w = v;                                   // the chunk's minimum of t[k] - k joins the carry
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                w = min(w, __shfl_xor(w, o, 64));
                m = min(m, __shfl_xor(m, o, 64));
            }
            carry = w;
            cmin = min(cmin, m);
        }
        for (int c = lane; c < V; c += 64) best[c] = cmin + 1;
        __syncthreads();
        for (int i = lane; i < ny; i += 64) {
            const long long c = y[i];
            if (c >= 0 && c < V) atomicMin(&best[c], cur[i]);
        }
        __syncthreads();
        const int r_eos = -cur[ny - 1];
        float* rw = rewards + ((size_t)j * B + b) * V;
        float* gn = gains + ((size_t)j * B + b) * V;
        for (int c = lane; c < V; c += 64) {
            const int r = c == eos ? r_eos : -best[c];
            rw[c] = (float)r;
            gn[c] = (float)(r - prev_pick);
        }
        const long long pj = pred[(size_t)j * B + b];
        prev_pick = (pj >= 0 && pj < V) ? (pj == eos ? r_eos : -best[pj]) : 0;
        __syncthreads();                                 // best / old are rewritten by the next column
    }
    for (int j = n; j < Lp; ++j) {
        float* rw = rewards + ((size_t)j * B + b) * V;
        float* gn = gains + ((size_t)j * B + b) * V;
        for (int c = lane; c < V; c += 64) { rw[c] = -1.f; gn[c] = -1000.f; }
    }
    if (pmask)
        for (int j = lane; j < Lp; j += 64) pmask[(size_t)j * B + b] = j < n ? 1.f : 0.f;
}

// mse_gain: rows are independent, one wave per row (as softmax_nll_kernel): g = max(gain, min_reward), cost = m sum_v (r - g)^2,
// dlogits = 2 m (r - g).  Lane-strided partial sums folded by the xor tree: a fixed order.
__global__ __launch_bounds__(256) void reward_mse_gain_kernel(const float* readouts, int ld, const float* gains, const float* mask, int n,
                                                              int V, float min_reward, float* cost, float* dlogits, int ldd) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= n) return;
    const float* x = readouts + (size_t)row * ld;
    const float* g = gains + (size_t)row * V;
    float* dl = dlogits + (size_t)row * ldd;
    const float m = mask ? mask[row] : 1.f;
    float s = 0.f;
    for (int v = lane; v < V; v += 64) {
        const float d = x[v] - fmaxf(g[v], min_reward);
        s += d * d;
        dl[v] = m == 0.f ? 0.f : 2.f * m * d;
    }
    s = wave_sum(s);
    if (lane == 0) cost[row] = m == 0.f ? 0.f : m * s;
}

// mse_reward: one work-group per utterance, one wave per label position at a time.  The predicted reward of row l adds
// P[l] = sum_{k=1..l} readouts[k, yhat[k]], so the gradient of row l's picked readout collects the error sums of all rows l' >= l;
// prefix and suffix sums run in label order on one thread (a fixed order; L is a few hundred at most).
__global__ __launch_bounds__(256) void reward_mse_reward_kernel(const float* readouts, int ld, const float* rewards, const long long* labels,
                                                                const float* mask, int L, int B, int V, float* cost, float* dlogits,
                                                                int ldd) {
    __shared__ float P[RM_MAX_L];
    __shared__ float E[RM_MAX_L];
    const int b = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    for (int l = tid; l < L; l += 256) {
        const long long c = labels[(size_t)l * B + b];
        P[l] = (l >= 1 && c >= 0 && c < V) ? readouts[((size_t)l * B + b) * ld + c] : 0.f;
    }
    __syncthreads();
    if (tid == 0) {
        float run = 0.f;
        for (int l = 0; l < L; ++l) { run += P[l]; P[l] = run; }
    }
    __syncthreads();
    for (int l = wave; l < L; l += 4) {
        const size_t row = (size_t)l * B + b;
        const float* x = readouts + row * ld;
        const float* tg = rewards + row * V;
        float* dl = dlogits + row * ldd;
        const float m = mask ? mask[row] : 1.f;
        const float p = P[l];
        float s = 0.f, es = 0.f;
        for (int v = lane; v < V; v += 64) {
            const float d = (x[v] + p) - tg[v];
            const float e = m == 0.f ? 0.f : 2.f * m * d;
            s += d * d;
            es += e;
            dl[v] = e;
        }
        s = wave_sum(s);
        es = wave_sum(es);
        if (lane == 0) {
            cost[row] = m == 0.f ? 0.f : m * s;
            E[l] = es;
        }
    }
    __syncthreads();
    if (tid == 0) {
        float run = 0.f;
        for (int l = L - 1; l >= 0; --l) { run += E[l]; E[l] = run; }
    }
    __syncthreads();
    for (int l = 1 + tid; l < L; l += 256) {
        const long long c = labels[(size_t)l * B + b];
        if (c >= 0 && c < V) dlogits[((size_t)l * B + b) * ldd + c] += E[l];
    }
}

extern "C" {

int lvsr_reward_gain(void* stream, const long long* groundtruth, int Lg, const long long* prediction, int Lp, int B, int eos, int V,
                     float* rewards, float* gains, float* prediction_mask) {
    LVSR_REQUIRE(groundtruth && prediction && rewards && gains, "lvsr_reward_gain: null argument");
    LVSR_REQUIRE(Lg > 0 && Lp > 0 && B > 0 && V > 0, "lvsr_reward_gain: bad sizes");
    LVSR_REQUIRE(Lg <= RG_MAX_Y && V <= RG_MAX_V,
                 "lvsr_reward_gain: sizes exceed the LDS budget (groundtruth positions <= RG_MAX_Y = %d, V <= RG_MAX_V = %d)", RG_MAX_Y,
                 RG_MAX_V);
    hipLaunchKernelGGL(reward_gain_kernel, dim3(B), dim3(64), 0, (hipStream_t)stream, groundtruth, Lg, prediction, Lp, B, (long long)eos,
                       V, rewards, gains, prediction_mask);
    return lvsr_check_launch("lvsr_reward_gain");
}

int lvsr_reward_mse(void* stream, int mode, const float* readouts, int ld, const float* gains, const float* rewards,
                    const long long* labels, const float* mask, int L, int B, int V, float min_reward, float* cost, float* dlogits,
                    int ldd) {
    LVSR_REQUIRE(mode == 0 || mode == 1, "lvsr_reward_mse: mode must be 0 (mse_gain) or 1 (mse_reward)");
    LVSR_REQUIRE(readouts && cost && dlogits && (mode == 0 ? gains != nullptr : (rewards && labels)), "lvsr_reward_mse: null argument");
    LVSR_REQUIRE(L > 0 && B > 0 && V > 0 && ld >= V && ldd >= V, "lvsr_reward_mse: bad sizes");
    LVSR_REQUIRE(mode == 0 || L <= RM_MAX_L, "lvsr_reward_mse: mse_reward holds at most RM_MAX_L = %d label positions in LDS", RM_MAX_L);
    if (mode == 0)
        hipLaunchKernelGGL(reward_mse_gain_kernel, dim3((L * B + 3) / 4), dim3(256), 0, (hipStream_t)stream, readouts, ld, gains, mask,
                           L * B, V, min_reward, cost, dlogits, ldd);
    else
        hipLaunchKernelGGL(reward_mse_reward_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, readouts, ld, rewards, labels, mask, L, B,
                           V, cost, dlogits, ldd);
    return lvsr_check_launch("lvsr_reward_mse");
}

}  // extern "C"
