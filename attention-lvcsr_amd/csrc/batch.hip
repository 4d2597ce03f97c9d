// Minibatch assembly on the device: the training set lives in HBM as one ragged store (frames and labels of all utterances back to
// back, 64-bit offset tables), and ONE launch writes the four padded, time-major tensors of a minibatch.
//
// Reference semantics: fuel `Padding` (libs/fuel/fuel/transformers/__init__.py:691-720), the switch of the first two axes and
// ForceCContiguous of the reference's stream (lvsr/datasets/__init__.py:303-309), which the reference (and Data.pad_batch) runs in
// host Python per minibatch.  Values are copied or are the constants 0 / 1: the outputs equal Data.pad_batch bit for bit.
//
// Every output element is written by exactly one thread, padding included (no memset in front).  One grid, three ranges of
// work-groups:
//   frames : a wave owns column b and BA_TCHUNK consecutive time steps; its 64 lanes run along the F contiguous floats of the
//            destination row (t, b) — 256 contiguous bytes per store instruction, the same for the source row of the store
//            (rows of one column are consecutive there).  The four waves of a work-group take neighbouring columns of the same
//            time steps, i.e. neighbouring destination rows.  The column's metadata (index, two offsets) is read once per wave.
//   recordings_mask : one thread per element of (T,B), lanes along b (contiguous).
//   labels, labels_mask : one thread per element of (L,B), lanes along b; the label reads are 8-byte gathers (L*B of them).
// An index outside [0, n) gives an empty column; an utterance longer than T (L) is cut there.  The host layer refuses both.
#include "common.h"
#include "lvsr_hip.h"

#define BA_THREADS 256
#define BA_TCHUNK 8            // time steps per wave of the frames range

// length (clamped to [0, cap]) and first element of utterance index[b] in a ragged table; an index outside the store: length 0
__device__ __forceinline__ int ba_span(const long long* off, const long long* index, int b, long long n, int cap, size_t* first) {
    const long long u = index[b];
    if (u < 0 || u >= n) { *first = 0; return 0; }
    const long long lo = off[u], len = off[u + 1] - lo;
    *first = (size_t)lo;
    return len <= 0 ? 0 : (len < cap ? (int)len : cap);
}

__global__ __launch_bounds__(BA_THREADS) void assemble_batch_kernel(const float* __restrict__ frames, const long long* __restrict__ frame_off,
                                                                    const long long* __restrict__ labels, const long long* __restrict__ label_off,
                                                                    const long long* __restrict__ index, long long n, int B, int T, int L, int F,
                                                                    unsigned frame_wgs, unsigned mask_wgs, float* __restrict__ rec,
                                                                    float* __restrict__ rmask, long long* __restrict__ olab,
                                                                    float* __restrict__ lmask) {
    const unsigned wg = blockIdx.x;
    if (wg < frame_wgs) {
        const size_t item = (size_t)wg * (BA_THREADS / 64) + (threadIdx.x >> 6);
        const int lane = threadIdx.x & 63;
        const int b = (int)(item % (size_t)B);
        const size_t t0 = item / (size_t)B * BA_TCHUNK;
        if (t0 >= (size_t)T) return;
        size_t first;
        const int len = ba_span(frame_off, index, b, n, T, &first);
        const size_t t1 = t0 + BA_TCHUNK < (size_t)T ? t0 + BA_TCHUNK : (size_t)T;
        for (size_t t = t0; t < t1; ++t) {
            float* dst = rec + (t * B + b) * F;
            if (t < (size_t)len) {
                const float* src = frames + (first + t) * (size_t)F;
                for (int c = lane; c < F; c += 64) dst[c] = src[c];
            } else {
                for (int c = lane; c < F; c += 64) dst[c] = 0.f;
            }
        }
        return;
    }
    if (wg < frame_wgs + mask_wgs) {
        const size_t e = (size_t)(wg - frame_wgs) * BA_THREADS + threadIdx.x;
        if (e >= (size_t)T * B) return;
        const int b = (int)(e % (size_t)B), t = (int)(e / (size_t)B);
        size_t first;
        rmask[e] = t < ba_span(frame_off, index, b, n, T, &first) ? 1.f : 0.f;
        return;
    }
    const size_t e = (size_t)(wg - frame_wgs - mask_wgs) * BA_THREADS + threadIdx.x;
    if (e >= (size_t)L * B) return;
    const int b = (int)(e % (size_t)B), l = (int)(e / (size_t)B);
    size_t first;
    const bool live = l < ba_span(label_off, index, b, n, L, &first);
    olab[e] = live ? labels[first + l] : 0;
    lmask[e] = live ? 1.f : 0.f;
}

extern "C" {

int lvsr_assemble_batch(void* stream, const lvsr_batch_args* a) {
    LVSR_REQUIRE(a, "lvsr_assemble_batch: null argument block");
    LVSR_REQUIRE(a->frames && a->frame_off && a->labels && a->label_off && a->index, "lvsr_assemble_batch: null store pointer");
    LVSR_REQUIRE(a->recordings && a->recordings_mask && a->out_labels && a->labels_mask, "lvsr_assemble_batch: null output pointer");
    LVSR_REQUIRE(a->n > 0, "lvsr_assemble_batch: the store holds no utterances (n = %lld)", a->n);
    LVSR_REQUIRE(a->B > 0 && a->T > 0 && a->L > 0 && a->F > 0, "lvsr_assemble_batch: bad sizes (B %d, T %d, L %d, F %d)", a->B, a->T,
                 a->L, a->F);
    const size_t B = (size_t)a->B, wave_items = B * (((size_t)a->T + BA_TCHUNK - 1) / BA_TCHUNK);
    const size_t frame_wgs = (wave_items + BA_THREADS / 64 - 1) / (BA_THREADS / 64);
    const size_t mask_wgs = ((size_t)a->T * B + BA_THREADS - 1) / BA_THREADS;
    const size_t label_wgs = ((size_t)a->L * B + BA_THREADS - 1) / BA_THREADS;
    LVSR_REQUIRE(frame_wgs + mask_wgs + label_wgs <= 0x7fffffffu, "lvsr_assemble_batch: minibatch too large for one grid (B %d, T %d, L %d)",
                 a->B, a->T, a->L);
    hipLaunchKernelGGL(assemble_batch_kernel, dim3((unsigned)(frame_wgs + mask_wgs + label_wgs)), dim3(BA_THREADS), 0, (hipStream_t)stream,
                       a->frames, a->frame_off, a->labels, a->label_off, a->index, a->n, a->B, a->T, a->L, a->F, (unsigned)frame_wgs,
                       (unsigned)mask_wgs, a->recordings, a->recordings_mask, a->out_labels, a->labels_mask);
    return lvsr_check_launch("lvsr_assemble_batch");
}

}  // extern "C"
