// ppo_kernels.hip -- PPO math kernels for MI355X (gfx950), C ABI in include/twoarmy_ppo.h.
//
// Everything here is HBM-bound elementwise / scan work on [T][N] rollout tensors; the conv/linear
// GEMMs of the actor-critic stay in PyTorch-ROCm (MIOpen / hipBLASLt on MFMA).  Reference arithmetic:
// soa/agent/PPO.py:73-92 (select_action), :112-115 (targets / advantages), :124-133 (losses).

#include <hip/hip_runtime.h>
#include <float.h>
#include <stdint.h>

#include <type_traits>

#include "launch.h"
#include "philox.h"
#include "twoarmy.h"
#include "twoarmy_ppo.h"
#include "visit_cell.h"

namespace {

constexpr float CAT_EPS = FLT_EPSILON;          // torch.finfo(float32).eps used by probs_to_logits

// ------------------------------------------------------------------ pieces the kernels below share
// One row of Categorical(probs = p): p[k] = row[k], returns S = sum p in ascending k; q = p / S is the caller's.
template <int A> __device__ __forceinline__ float cat_row(const float *__restrict__ row, float (&p)[A]) {
    float S = 0.f;
#pragma unroll
    for (int k = 0; k < A; ++k) { p[k] = row[k]; S += p[k]; }
    return S;
}
__device__ __forceinline__ float cat_log(float q) { return logf(fminf(fmaxf(q, CAT_EPS), 1.0f - CAT_EPS)); }

// Sum of K values per thread over a 256-thread workgroup: the tree 128, 64, ... 1 on lds[K][256], every level adding
// element tid + s to element tid (a fixed shape: the sums' bits are part of the contract).  v holds the sums afterwards.
template <typename T, int K> __device__ __forceinline__ void block_sum(T (&v)[K], T *lds) {
    const int tid = threadIdx.x;
#pragma unroll
    for (int k = 0; k < K; ++k) lds[k * 256 + tid] = v[k];
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) {
#pragma unroll
            for (int k = 0; k < K; ++k) lds[k * 256 + tid] += lds[k * 256 + tid + s];
        }
        __syncthreads();
    }
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = lds[k * 256];
}

__device__ __forceinline__ float4 relu4(float4 v) {
    return make_float4(fmaxf(v.x, 0.f), fmaxf(v.y, 0.f), fmaxf(v.z, 0.f), fmaxf(v.w, 0.f));
}
__device__ __forceinline__ float4 mask4(float4 g, float4 y) {       // g where y > 0 (ReLU backward)
    return make_float4(y.x > 0.f ? g.x : 0.f, y.y > 0.f ? g.y : 0.f, y.z > 0.f ? g.z : 0.f, y.w > 0.f ? g.w : 0.f);
}
__device__ __forceinline__ void add4(float4 &acc, const float4 &o) { acc.x += o.x; acc.y += o.y; acc.z += o.z; acc.w += o.w; }
__device__ __forceinline__ float4 fma4(float x, float4 w, float4 acc) {
    return make_float4(fmaf(x, w.x, acc.x), fmaf(x, w.y, acc.y), fmaf(x, w.z, acc.z), fmaf(x, w.w, acc.w));
}

// red[rows][stride] holds one float4 per pixel slot and channel quad: slot 0 plus slots 1 .. rows - 1, in that order.
__device__ __forceinline__ float4 slot_sum4(const float4 *red, int rows, int stride, int cq) {
    float4 sum = red[cq];
    for (int r = 1; r < rows; ++r) add4(sum, red[r * stride + cq]);
    return sum;
}

// "the episode ends at step i", non-zero for either flag
__device__ __forceinline__ uint32_t done_at(const uint8_t *__restrict__ terminated, const uint8_t *__restrict__ truncated,
                                            size_t i) {
    return (uint32_t)(terminated[i] | truncated[i]);
}

// ------------------------------------------------------------------ categorical sample
template <int A>
__global__ void ppo_sample_kernel(const float *__restrict__ probs, int B, const float *__restrict__ uniforms,
                                  uint32_t k0, uint32_t k1, uint64_t offset, const uint64_t *__restrict__ offset_dev,
                                  int32_t *__restrict__ action, float *__restrict__ logp) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    float p[A];
    const float sum = cat_row<A>(probs + (size_t)b * A, p);
    float u;
    if (uniforms) u = uniforms[b];
    else {
        const uint64_t ctr = (uint64_t)b + offset + (offset_dev ? *offset_dev : 0ull);
        uint32_t c0 = (uint32_t)ctr, c1 = (uint32_t)(ctr >> 32), c2 = 0, c3 = 0x54574F53u;   // 'TWOS'
        philox4x32_10(k0, k1, c0, c1, c2, c3);
        u = (float)(c0 >> 8) * (1.0f / 16777216.0f);       // 24 random bits -> [0, 1)
    }
    // the rounded cumsum can end below u (up to 1 - 2^-24): then the last action with q > 0, never a zero-probability one
    int a = A - 1, last = A - 1;
    float cum = 0.f, qa = 0.f;
    bool found = false;
#pragma unroll
    for (int k = 0; k < A; ++k) {
        const float q = p[k] / sum;
        cum += q;
        if (q > 0.f) last = k;
        if (!found && cum > u) { a = k; found = true; }
    }
    if (!found) a = last;
#pragma unroll
    for (int k = 0; k < A; ++k) if (k == a) qa = p[k] / sum;
    action[b] = a;
    logp[b] = cat_log(qa);
}

// ------------------------------------------------------------------ conv epilogues (channels-last activations)
// The conv GEMMs stay in MIOpen; what PyTorch wraps around each of them -- output.add_(bias) (one pass), ReLU
// (another pass), and in backward threshold_backward (one pass) + the bias-gradient reduction (one pass) -- are pure
// HBM passes over the biggest tensors of the update (33x33x64 floats per sample after conv1).  These two kernels do
// each pair in ONE pass.  Activations are channels-last: element i belongs to channel i % C, C % 4 == 0.
__global__ __launch_bounds__(256) void ppo_bias_relu_kernel(float4 *__restrict__ y, const float4 *__restrict__ bias,
                                                            size_t n4, int c4) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
        float4 v = y[i];
        add4(v, bias[i % c4]);
        y[i] = relu4(v);
    }
}

// gx = gy * (y > 0), partial[block][C] = sum over the block's pixels of gx.  Block = 256 threads laid out as
// (256 / c4) pixel rows x c4 channel quads, walking `pixels_per_block` consecutive pixels; the per-thread sums are
// combined through LDS in a fixed order (deterministic), the caller adds the per-block partials.
__global__ __launch_bounds__(256) void ppo_relu_bwd_bias_grad_kernel(const float4 *__restrict__ gy,
                                                                     const float4 *__restrict__ y,
                                                                     float4 *__restrict__ gx,
                                                                     float4 *__restrict__ partial, size_t n_pixels,
                                                                     int c4, int pixels_per_block) {
    __shared__ float4 red[256];
    const int rows = 256 / c4;                        // pixel rows handled side by side (c4 <= 64)
    const int cq = threadIdx.x % c4, row = threadIdx.x / c4;
    const size_t p0 = (size_t)blockIdx.x * pixels_per_block;
    const size_t p1 = p0 + pixels_per_block < n_pixels ? p0 + pixels_per_block : n_pixels;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    if (row < rows) {
        for (size_t px = p0 + row; px < p1; px += rows) {
            const size_t i = px * c4 + cq;
            const float4 o = mask4(gy[i], y[i]);
            gx[i] = o;
            add4(acc, o);
        }
    }
    red[threadIdx.x] = acc;
    __syncthreads();
    if (row == 0) partial[(size_t)blockIdx.x * c4 + cq] = slot_sum4(red, rows, c4, cq);
}

// ------------------------------------------------------------------ conv1 of TINet, fused with its input upsampling
// all_net.py:146,176-186: frames (B, F, 17, 17) -> UpsamplingNearest2d(x4) -> Conv2d(F -> 64, k4, s2) -> ReLU = (B, 64, 33, 33).
// Output row oy reads upsampled rows 2oy .. 2oy+3, i.e. source row m = oy >> 1 for all four taps when oy is even and
// source rows m, m+1 (two taps each) when oy is odd; the same for columns.  So the layer is a 2x2-tap convolution
// of the 17x17 frame whose weights depend on the output's (row, column) parity -- 16x fewer input bytes, no 68x68
// tensor, and the bias add and ReLU happen before the one and only store of the layer's (largest) activation.
// Folded weights wf[py][px][ty][tx][c][64] (taps that a parity does not have carry zeros) come from the caller.
// Block = 256 threads = 16 channel quads x 16 pixel slots, one sample per block; per parity phase the thread keeps its
// 4 taps x F x float4 weights in registers and walks the phase's pixels; x values are LDS broadcasts.
// One sample's frames src[F][17][17] -> xs[F][18][18]: row / column 17 = zero pad for the (unused) far taps.
template <int F> __device__ __forceinline__ void conv1_stage_frame(float *xs, const float *__restrict__ src, int tid) {
    for (int i = tid; i < F * 324; i += 256) {
        const int c = i / 324, r = i - c * 324, y = r / 18, x = r - y * 18;
        xs[i] = (y < 17 && x < 17) ? src[c * 289 + y * 17 + x] : 0.f;
    }
}

template <int F, int CQ>                           // F input channels, CQ = output channels / 4 (16 for TINet, 4 for Net_Encoder)
__global__ __launch_bounds__(256) void ppo_conv1_up4_kernel(const float *__restrict__ frames, const float4 *__restrict__ wf,
                                                            const float4 *__restrict__ bias, float4 *__restrict__ out, int B) {
    __shared__ float xs[F * 18 * 18];
    constexpr int SLOTS = 256 / CQ;
    const int b = blockIdx.x, tid = threadIdx.x;
    const int cq = tid % CQ, slot = tid / CQ;
    conv1_stage_frame<F>(xs, frames + (size_t)b * F * 289, tid);
    __syncthreads();
    const float4 bv = bias[cq];
    float4 *dst = out + (size_t)b * 1089 * CQ;
#pragma unroll 1
    for (int ph = 0; ph < 4; ++ph) {
        const int py = ph >> 1, px = ph & 1;
        float4 w[4 * F];
#pragma unroll
        for (int k = 0; k < 4 * F; ++k) w[k] = wf[(ph * 4 * F + k) * CQ + cq];      // [ty][tx][c] -> k = (ty*2+tx)*F + c
        const int ny = 17 - py, nx = 17 - px;               // output rows / columns of this parity
        for (int q = slot; q < ny * nx; q += SLOTS) {
            const int m = q / nx, n = q - m * nx;
            float4 acc = bv;
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const int ty = t >> 1, tx = t & 1;
#pragma unroll
                for (int c = 0; c < F; ++c) acc = fma4(xs[c * 324 + (m + ty) * 18 + n + tx], w[t * F + c], acc);
            }
            dst[((2 * m + py) * 33 + 2 * n + px) * CQ + cq] = relu4(acc);
        }
    }
}

// Backward of the fused first layer: gw_folded[py][px][ty][tx][c][64] = sum over samples and over the output pixels of
// parity (py, px) of x[c][m+ty][n+tx] * g[pixel][64], g = gy where the layer's output y is positive (ReLU), and the bias
// gradient sum of g -- gy and y are read exactly once, nothing else of the 33x33x64 size is touched (the separate
// ReLU-backward pass + MIOpen weight-gradient conv on re-upsampled frames read and wrote it four times).
// Grid = (groups, 4 parities); a block walks samples blockIdx.x, +groups, ...; block = 16 channel quads x 16 pixel slots,
// 4 taps x F float4 accumulators per thread, combined over the 16 slots through LDS in a fixed order; per-block partial
// sums (deterministic), the caller adds the groups.
template <int F>
__global__ __launch_bounds__(256) void ppo_conv1_up4_bwd_kernel(const float *__restrict__ frames, const float4 *__restrict__ gy,
                                                                const float4 *__restrict__ y, float4 *__restrict__ gw_part,
                                                                float4 *__restrict__ gb_part, int B) {
    __shared__ float xs[F * 18 * 18];
    __shared__ float4 red[256];
    const int tid = threadIdx.x, cq = tid & 15, slot = tid >> 4;
    const int ph = blockIdx.y, py = ph >> 1, px = ph & 1;
    const int ny = 17 - py, nx = 17 - px;
    float4 acc[4 * F];
#pragma unroll
    for (int k = 0; k < 4 * F; ++k) acc[k] = make_float4(0.f, 0.f, 0.f, 0.f);
    float4 accb = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int b = blockIdx.x; b < B; b += gridDim.x) {
        __syncthreads();                                    // the previous sample's xs is no longer read
        conv1_stage_frame<F>(xs, frames + (size_t)b * F * 289, tid);
        __syncthreads();
        const size_t base = (size_t)b * 1089 * 16;
        for (int q = slot; q < ny * nx; q += 16) {
            const int m = q / nx, n = q - m * nx;
            const size_t o = base + (size_t)((2 * m + py) * 33 + 2 * n + px) * 16 + cq;
            const float4 g = mask4(gy[o], y[o]);
            add4(accb, g);
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const int ty = t >> 1, tx = t & 1;
#pragma unroll
                for (int c = 0; c < F; ++c) acc[t * F + c] = fma4(xs[c * 324 + (m + ty) * 18 + n + tx], g, acc[t * F + c]);
            }
        }
    }
    // combine the 16 pixel slots (fixed order), one accumulator at a time
    const size_t wbase = ((size_t)blockIdx.x * 4 + ph) * (4 * F) * 16;
#pragma unroll
    for (int k = 0; k <= 4 * F; ++k) {
        __syncthreads();
        red[tid] = k < 4 * F ? acc[k < 4 * F ? k : 0] : accb;
        __syncthreads();
        if (slot == 0) {
            const float4 sum = slot_sum4(red, 16, 16, cq);
            if (k < 4 * F) gw_part[wbase + (size_t)k * 16 + cq] = sum;
            else gb_part[((size_t)blockIdx.x * 4 + ph) * 16 + cq] = sum;
        }
    }
}

// ------------------------------------------------------------------ GAE: segmented reverse scan
// Block = 256 threads = 4 waves, GN envs (columns) x chunks of 64 time steps walked from T backwards (GN = 16 for
// N < 16384 so that a 4096-env rollout still fills 256 workgroups; 64 otherwise).
// Lanes of a wave are TIME within one env column: A_t = d_t + c_t * A_{t+1} is the suffix composition
// of affine maps (c, d), computed with a 6-step Kogge-Stone over __shfl_down; the running A of the
// chunk above enters as the carry.  Tiles go through LDS so that global accesses stay coalesced.
constexpr int GT = 64;     // time steps per chunk

template <int GN>          // envs per block
__global__ __launch_bounds__(256) void ppo_gae_kernel(const float *__restrict__ reward, const float *__restrict__ value,
                                                      const float *__restrict__ next_value,
                                                      const uint8_t *__restrict__ done, float gamma, float lambda,
                                                      int use_done_mask, int T, int N, float *__restrict__ adv,
                                                      float *__restrict__ target, float *__restrict__ ret) {
    __shared__ float sd[GT][GN + 1];
    __shared__ float sc[GT][GN + 1];
    __shared__ float carry[GN];
    constexpr int ROWS = 256 / GN;                      // time rows loaded / stored per pass
    const int tid = threadIdx.x, tx = tid % GN, ty = tid / GN;
    const int n = blockIdx.x * GN + tx;
    if (tid < GN) carry[tid] = 0.f;
    const int nchunks = (T + GT - 1) / GT;
    for (int ch = nchunks - 1; ch >= 0; --ch) {
        const int t0 = ch * GT;
        __syncthreads();
        for (int r = ty; r < GT; r += ROWS) {
            const int t = t0 + r;
            float d = 0.f, c = 1.f;                     // identity map for rows past T
            if (t < T && n < N) {
                const size_t i = (size_t)t * N + n;
                const float cut = (use_done_mask && done[i]) ? 0.f : 1.f;
                // same rounding sequence as torch: g*V, * cut, + r, - V.  cut is 0 or 1, so a contracted
                // fma(cut, g*V, r) rounds exactly like the separate multiply and add.
                const float tv = reward[i] + (gamma * next_value[i]) * cut;
                if (target) target[i] = tv;
                d = tv - value[i];
                c = gamma * lambda * cut;
            }
            sd[r][tx] = d; sc[r][tx] = c;
        }
        __syncthreads();
        const int wave = tid >> 6, lane = tid & 63;     // lane = time row inside the chunk
        for (int e = wave * (GN / 4); e < (wave + 1) * (GN / 4); ++e) {
            float d = sd[lane][e], c = sc[lane][e];
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) {
                const float d2 = __shfl_down(d, off), c2 = __shfl_down(c, off);
                // c == 0 (lambda = 0 or a done) ends the segment: (0, d) absorbs whatever follows, and skipping the
                // combine keeps 0 * inf / 0 * NaN of a later step out of it
                if (lane + off < 64 && c != 0.f) { d = fmaf(c, d2, d); c = c * c2; }
            }
            const float a = c != 0.f ? fmaf(c, carry[e], d) : d;     // A of this row given the chunk above
            sd[lane][e] = a;
            const float a0 = __shfl(a, 0);
            if (lane == 0) carry[e] = a0;               // only this wave touches carry[e]
        }
        __syncthreads();
        for (int r = ty; r < GT; r += ROWS) {
            const int t = t0 + r;
            if (t < T && n < N) {
                const size_t i = (size_t)t * N + n;
                const float a = sd[r][tx];
                if (adv) adv[i] = a;
                if (ret) ret[i] = a + value[i];
            }
        }
    }
}

// ------------------------------------------------------------------ GAE along a flat record array, cut at run ends
// The records of ppo_her_relabel come as runs; A_j = d_j + c_j * A_{j+1} with c_j = 0 at a run end is again a suffix
// composition of affine maps, now along ONE array of H records, so it is scanned as a tree over workgroups instead of
// by one wavefront per column: a workgroup owns GR_BLOCK = 2048 consecutive records, each of its 4 wavefronts
// GR_CHUNKS = 8 chunks of 64 (coalesced: lane = record inside the chunk), scanned by gae_suffix_scan and folded from
// the last chunk to the first.  Level 0 are the records, level l + 1 the composites of the workgroups of level l:
//   reduce  level l -> the composite (c, d) of every workgroup, written to level l + 1      (while a level has > 2048 maps)
//   apply   the top level from x = 0, then every level below it with x of workgroup b + 1 (level l + 1, already applied)
//           as the value that enters workgroup b from behind
// H <= 2048: one launch; H <= 2048^2: three.  Every combine keeps the c != 0 guard, so a map with c = 0 hands its d on
// exactly and nothing behind it is looked at.
constexpr int GR_CHUNKS = 8;
constexpr int GR_WAVE = 64 * GR_CHUNKS;
constexpr int GR_BLOCK = 4 * GR_WAVE;
constexpr int GR_MAX_LEVELS = 4;                    // 2048^4 > 2^40 records

// The shuffle step of ppo_gae_kernel as a function (that kernel keeps its own loop: its code is pinned, section 6.26 of
// DESIGN.md): on entry lane l holds the map x -> d + c * x of its element, on exit the composite of the elements l .. 63.
__device__ __forceinline__ void gae_suffix_scan(float &c, float &d, int lane) {
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const float d2 = __shfl_down(d, off), c2 = __shfl_down(c, off);
        if (lane + off < 64 && c != 0.f) { d = fmaf(c, d2, d); c = c * c2; }     // c == 0 ends the segment, as there
    }
}

// first o behind: the map of (c, d) followed by (C, D), kept in (C, D)
__device__ __forceinline__ void gr_compose(float c, float d, float &C, float &D) {
    if (c != 0.f) { D = fmaf(c, D, d); C = c * C; }
    else { D = d; C = 0.f; }
}
__device__ __forceinline__ float gr_eval(float c, float d, float x) { return c != 0.f ? fmaf(c, x, d) : d; }

struct gr_records {                                 // level 0: the maps come from the records, the scan goes to adv / ret
    const float *reward, *value, *next_value;
    const uint8_t *done, *run_end;
    float gamma, lambda;
    int use_done_mask;
    float *adv, *target, *ret;
    __device__ __forceinline__ void load(int64_t i, int64_t n, bool write, float &c, float &d) const {
        c = 1.f; d = 0.f;                           // identity behind the last record
        if (i < n) {
            const float cut = (use_done_mask && done[i]) ? 0.f : 1.f;
            const float tv = reward[i] + (gamma * next_value[i]) * cut;      // ppo_gae_kernel's rounding sequence
            if (write && target) target[i] = tv;
            d = tv - value[i];
            c = (run_end[i] || i == n - 1) ? 0.f : gamma * lambda * cut;
        }
    }
    __device__ __forceinline__ void store(int64_t i, float a) const {
        if (adv) adv[i] = a;
        if (ret) ret[i] = a + value[i];
    }
};
struct gr_composites {                              // level >= 1: (c[i], d[i]) in the workspace; x replaces d in place
    const float *c;
    float *d;
    __device__ __forceinline__ void load(int64_t i, int64_t n, bool, float &cc, float &dd) const {
        cc = 1.f; dd = 0.f;
        if (i < n) { cc = c[i]; dd = d[i]; }
    }
    __device__ __forceinline__ void store(int64_t i, float x) const { d[i] = x; }
};

template <typename Src>
__global__ __launch_bounds__(256) void ppo_gae_runs_reduce_kernel(Src src, int64_t n, float *__restrict__ out_c,
                                                                  float *__restrict__ out_d) {
    __shared__ float wc[4], wd[4];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int64_t base = (int64_t)blockIdx.x * GR_BLOCK + wave * GR_WAVE;
    float C = 1.f, D = 0.f;                         // composite of the chunks behind the current one
#pragma unroll
    for (int q = GR_CHUNKS - 1; q >= 0; --q) {
        float c, d;
        src.load(base + q * 64 + lane, n, false, c, d);
        gae_suffix_scan(c, d, lane);
        gr_compose(__shfl(c, 0), __shfl(d, 0), C, D);
    }
    if (lane == 0) { wc[wave] = C; wd[wave] = D; }
    __syncthreads();
    if (tid == 0) {
        C = wc[3]; D = wd[3];                       // the four wavefronts, last to first
        for (int w = 2; w >= 0; --w) gr_compose(wc[w], wd[w], C, D);
        out_c[blockIdx.x] = C; out_d[blockIdx.x] = D;
    }
}

template <typename Src>
__global__ __launch_bounds__(256) void ppo_gae_runs_apply_kernel(Src src, int64_t n, const float *__restrict__ carry_x,
                                                                 int64_t n_carry) {
    __shared__ float wc[4], wd[4];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int64_t base = (int64_t)blockIdx.x * GR_BLOCK + wave * GR_WAVE;
    float cs[GR_CHUNKS], ds[GR_CHUNKS];             // suffix composites inside each chunk, kept for the second walk
    float C = 1.f, D = 0.f;
#pragma unroll
    for (int q = GR_CHUNKS - 1; q >= 0; --q) {
        src.load(base + q * 64 + lane, n, true, cs[q], ds[q]);
        gae_suffix_scan(cs[q], ds[q], lane);
        gr_compose(__shfl(cs[q], 0), __shfl(ds[q], 0), C, D);
    }
    if (lane == 0) { wc[wave] = C; wd[wave] = D; }
    __syncthreads();
    // what enters this wavefront from behind: the next workgroup's value pushed through the wavefronts in between
    const int64_t nb = (int64_t)blockIdx.x + 1;
    float x = (carry_x && nb < n_carry) ? carry_x[nb] : 0.f;
    for (int w = 3; w > wave; --w) x = gr_eval(wc[w], wd[w], x);
#pragma unroll
    for (int q = GR_CHUNKS - 1; q >= 0; --q) {
        const float a = gr_eval(cs[q], ds[q], x);
        const int64_t i = base + q * 64 + lane;
        if (i < n) src.store(i, a);
        x = __shfl(a, 0);
    }
}

// link_j of the header, four records per thread; the out-of-pattern count as one integer atomic per wavefront
__global__ __launch_bounds__(256) void ppo_run_ends_kernel(const int32_t *__restrict__ t, const int32_t *__restrict__ n,
                                                           const float *__restrict__ goal, const uint8_t *__restrict__ done,
                                                           int64_t H, uint8_t *__restrict__ run_end,
                                                           int32_t *__restrict__ broken) {
    int count = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int64_t j = ((int64_t)blockIdx.x * 4 + k) * 256 + threadIdx.x;
        bool brk = false;
        if (j < H) {
            const bool dn = done[j] != 0;
            bool link = false;
            if (!dn && j + 1 < H)                   // nothing at index H is read
                link = n[j + 1] == n[j] && (int64_t)t[j + 1] == (int64_t)t[j] + 1 && goal[2 * j + 2] == goal[2 * j] &&
                       goal[2 * j + 3] == goal[2 * j + 1];
            run_end[j] = link ? 0 : 1;
            brk = !dn && !link;
        }
        count += __popcll(__ballot(brk));
    }
    if (broken && (threadIdx.x & 63) == 0 && count) atomicAdd(broken, count);
}

// ------------------------------------------------------------------ advantage normalisation
__global__ __launch_bounds__(256) void ppo_moments_kernel(const float *__restrict__ x, int64_t n, double *__restrict__ ws) {
    __shared__ double lds[2 * 256];
    double m[2] = {0.0, 0.0};                                                      // sum x, sum x^2
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const double v = (double)x[i];
        m[0] += v; m[1] += v * v;
    }
    block_sum(m, lds);
    if (threadIdx.x == 0) { ws[2 * blockIdx.x] = m[0]; ws[2 * blockIdx.x + 1] = m[1]; }
}

__global__ __launch_bounds__(256) void ppo_normalise_kernel(float *__restrict__ x, int64_t n, float eps,
                                                            const double *__restrict__ ws, int nblocks) {
    __shared__ float s_mean, s_inv;
    __shared__ double lds[2 * 256];
    double m[2];                                                                   // nblocks <= 256 partial sums
    m[0] = (int)threadIdx.x < nblocks ? ws[2 * threadIdx.x] : 0.0;
    m[1] = (int)threadIdx.x < nblocks ? ws[2 * threadIdx.x + 1] : 0.0;
    block_sum(m, lds);                                                             // fixed-order tree: deterministic
    if (threadIdx.x == 0) {
        const double a = m[0], b = m[1];
        const double mean = a / (double)n;
        double var = n > 1 ? (b - (double)n * mean * mean) / (double)(n - 1) : 0.0;  // unbiased
        if (var < 0.0) var = 0.0;
        s_mean = (float)mean;
        s_inv = 1.0f / ((float)sqrt(var) + eps);
    }
    __syncthreads();
    const float mean = s_mean, inv = s_inv;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256)
        x[i] = (x[i] - mean) * inv;
}

// ------------------------------------------------------------------ fused PPO losses, forward + backward
// The update diagnostics of ppo_loss_fwd_bwd_stats (twoarmy_ppo.h): LS_NV per-row accumulators, every one a sum but
// LS_MAX.  A row that is padding holds the identity (+0.0 everywhere: |ratio - 1| is never negative), and adding the
// identity changes no bit of a partial, so neither the padding nor the number of workgroups reaches `stats`.
constexpr int LS_NV = 12, LS_MAX = 5, LS_CALLS = 12;

__device__ __forceinline__ void ls_combine(double (&v)[LS_NV], const double (&w)[LS_NV]) {
#pragma unroll
    for (int k = 0; k < LS_NV; ++k) v[k] = k == LS_MAX ? fmax(v[k], w[k]) : v[k] + w[k];
}

// The 64 lanes of a wavefront as a binary tree in lane order (the shape of ep_wave_reduce); lane 0 ends with all 64.
__device__ __forceinline__ void ls_wave_reduce(double (&v)[LS_NV]) {
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) {
        double w[LS_NV];
#pragma unroll
        for (int k = 0; k < LS_NV; ++k) w[k] = __shfl_down(v[k], s, 64);
        ls_combine(v, w);
    }
}

// STATS = false is ppo_loss_fwd_bwd[_masked]'s kernel: `sws` is not read and every statement under `if constexpr (STATS)`
// is gone, so its bits and its registers are those it had before the diagnostics came.
template <int A, bool STATS>
__global__ __launch_bounds__(256) void ppo_loss_kernel(const float *__restrict__ probs, const int32_t *__restrict__ action,
                                                       const float *__restrict__ old_logp, const float *__restrict__ adv,
                                                       const float *__restrict__ value, const float *__restrict__ target_v,
                                                       int B, int n_valid, float clip, float ent_coef,
                                                       float *__restrict__ grad_probs, float *__restrict__ grad_value,
                                                       float *__restrict__ ws, double *__restrict__ sws) {
    __shared__ float lds[2 * 256];
    const int b = blockIdx.x * 256 + threadIdx.x;
    float la = 0.f, lv = 0.f;
    [[maybe_unused]] double st[LS_NV];
    if constexpr (STATS) {
#pragma unroll
        for (int k = 0; k < LS_NV; ++k) st[k] = 0.0;
    }
    if (b >= n_valid && b < B) {                      // padding rows of a fixed-shape minibatch: no loss, no gradient
#pragma unroll
        for (int k = 0; k < A; ++k) grad_probs[(size_t)b * A + k] = 0.f;
        grad_value[b] = 0.f;
    }
    if (b < n_valid) {
        const float invB = 1.0f / (float)n_valid;
        float p[A], q[A], l[A];
        bool inside[A];
        const float S = cat_row<A>(probs + (size_t)b * A, p);
        float H = 0.f;
#pragma unroll
        for (int k = 0; k < A; ++k) {
            q[k] = p[k] / S;
            inside[k] = q[k] >= CAT_EPS && q[k] <= 1.0f - CAT_EPS;        // clamp passes gradient inside (inclusive)
            l[k] = cat_log(q[k]);
            H -= q[k] * l[k];
        }
        const int a = action[b];
        float la_logp = 0.f;
#pragma unroll
        for (int k = 0; k < A; ++k) if (k == a) la_logp = l[k];
        const float lr = la_logp - old_logp[b];
        const float ratio = expf(lr);
        const float ad = adv[b];
        const float lo = 1.0f - clip, hi = 1.0f + clip;
        const float s1 = ratio * ad;
        const float s2 = fminf(fmaxf(ratio, lo), hi) * ad;
        la = -fminf(s1, s2) - ent_coef * H;
        // d/d(ratio) of min(s1, s2): torch.minimum splits ties; clamp passes gradient on [lo, hi]
        const bool in_clip = ratio >= lo && ratio <= hi;
        float w1 = s1 < s2 ? 1.f : (s1 == s2 ? 0.5f : 0.f);
        float w2 = s2 < s1 ? 1.f : (s1 == s2 ? 0.5f : 0.f);
        const float g_ratio = -(w1 + (in_clip ? w2 : 0.f)) * ad;
        const float g_logp = g_ratio * ratio;
        // gradient w.r.t. normalised q, then through q = p / S
        float gq[A];
        float dot = 0.f;
#pragma unroll
        for (int k = 0; k < A; ++k) {
            float g = (k == a && inside[k]) ? g_logp / q[k] : 0.f;
            g += ent_coef * (l[k] + (inside[k] ? 1.f : 0.f));            // -ent_coef * dH/dq_k
            gq[k] = g;
            dot += g * q[k];
        }
#pragma unroll
        for (int k = 0; k < A; ++k) grad_probs[(size_t)b * A + k] = (gq[k] - dot) / S * invB;
        // SmoothL1 (beta = 1)
        const float d = value[b] - target_v[b];
        const float ab = fabsf(d);
        lv = ab < 1.0f ? 0.5f * d * d : ab - 0.5f;
        grad_value[b] = (ab < 1.0f ? d : (d > 0.f ? 1.f : -1.f)) * invB;
        if constexpr (STATS) {                        // the row's diagnostics, from the float32 values above (twoarmy_ppo.h)
            bool in_a = false;
            float top = q[0];
#pragma unroll
            for (int k = 0; k < A; ++k) {
                if (k == a) in_a = inside[k];
                top = fmaxf(top, q[k]);
            }
            const double t = (double)target_v[b], e = (double)(target_v[b] - value[b]);
            const double dev = (double)ratio - 1.0;
            st[0] = 1.0;
            st[1] = (double)H;
            st[2] = (double)lr;
            st[3] = dev - (double)lr;                 // (r - 1) - log r in double: nothing is lost near r = 1
            st[4] = (ratio < lo || ratio > hi) ? 1.0 : 0.0;
            st[LS_MAX] = fabs(dev);
            st[6] = t;
            st[7] = t * t;
            st[8] = e;
            st[9] = e * e;
            st[10] = in_a ? 0.0 : 1.0;
            st[11] = (double)top;
        }
    }
    float sums[2] = {la, lv};
    block_sum(sums, lds);
    if (threadIdx.x == 0) { ws[2 * blockIdx.x] = sums[0]; ws[2 * blockIdx.x + 1] = sums[1]; }
    if constexpr (STATS) {                            // lanes in order, then the four wavefronts in order
        __shared__ double sh[4][LS_NV];
        ls_wave_reduce(st);
        const int wave = threadIdx.x >> 6;
        if ((threadIdx.x & 63) == 0) {
#pragma unroll
            for (int k = 0; k < LS_NV; ++k) sh[wave][k] = st[k];
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            for (int w = 1; w < 4; ++w) {
                double o[LS_NV];
#pragma unroll
                for (int k = 0; k < LS_NV; ++k) o[k] = sh[w][k];
                ls_combine(st, o);
            }
#pragma unroll
            for (int k = 0; k < LS_NV; ++k) sws[(size_t)blockIdx.x * LS_NV + k] = st[k];
        }
    }
}

__device__ __forceinline__ void loss_means(const float *__restrict__ ws, int nblocks, int B, float *__restrict__ losses) {
    float a = 0.f, v = 0.f;
    for (int k = 0; k < nblocks; ++k) { a += ws[2 * k]; v += ws[2 * k + 1]; }           // fixed order
    losses[0] = a / (float)B;
    losses[1] = v / (float)B;
}

__global__ void ppo_loss_finalize_kernel(const float *__restrict__ ws, int nblocks, int B, float *__restrict__ losses) {
    if (threadIdx.x == 0 && blockIdx.x == 0) loss_means(ws, nblocks, B, losses);
}

// The final pass of ppo_loss_fwd_bwd_stats, one wavefront: the losses as above, and stats += the partials.  Lane l folds
// the partials l, l + 64, l + 128, ... one after the other from the identity, the lanes are combined in lane order: which
// partials meet at which node depends on their index alone, never on nblocks, so the all-identity partials of padding
// workgroups leave every bit as it is.  The identity is +0.0, hence no sum that reaches stats is -0.0.
__global__ __launch_bounds__(64) void ppo_loss_stats_finalize_kernel(const float *__restrict__ ws,
                                                                    const double *__restrict__ sws, int nblocks, int B,
                                                                    float *__restrict__ losses, double *__restrict__ stats) {
    const int lane = threadIdx.x;
    if (lane == 0) loss_means(ws, nblocks, B, losses);
    double v[LS_NV];
#pragma unroll
    for (int k = 0; k < LS_NV; ++k) v[k] = 0.0;
    for (int blk = lane; blk < nblocks; blk += 64) {
        double o[LS_NV];
#pragma unroll
        for (int k = 0; k < LS_NV; ++k) o[k] = sws[(size_t)blk * LS_NV + k];
        ls_combine(v, o);
    }
    ls_wave_reduce(v);
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < LS_NV; ++k) stats[k] = k == LS_MAX ? fmax(stats[k], v[k]) : stats[k] + v[k];
        stats[LS_CALLS] += 1.0;
    }
}

// ------------------------------------------------------------------ shortest-path prior: set-valued imitation term
// One row of the prior (twoarmy_ppo.h): S = sum p, q = p / S, m = the mass on the masked actions summed in ascending a,
// rest = the mass on the others (the upper clamp is decided on `rest`, which is accurate where m is within rounding of
// 1), top = arg-max of q, lowest index on ties.
template <int A> struct prior_row_t { float S, m, rest; int top; };
template <int A> __device__ __forceinline__ prior_row_t<A> prior_row(const float *__restrict__ p, uint32_t mask)
{
    float v[A];
    const float S = cat_row<A>(p, v);
    prior_row_t<A> r = {S, 0.f, 0.f, 0};
    float best = 0.f;
#pragma unroll
    for (int k = 0; k < A; ++k) {
        const float q = v[k] / S;
        if ((mask >> k) & 1u) r.m += q; else r.rest += q;
        if (k == 0 || q > best) { best = q; r.top = k; }
    }
    return r;
}

// pass 1: per-workgroup partial sums {loss, mass} and counts {labelled, arg-max in the mask} -> ws[4 * block]
struct prior_sums_t {
    float l, m;
    int lab, agree;
    __device__ __forceinline__ prior_sums_t &operator+=(const prior_sums_t &o) {
        l += o.l; m += o.m; lab += o.lab; agree += o.agree;
        return *this;
    }
};

template <int A>
__global__ __launch_bounds__(256) void ppo_prior_partial_kernel(const float *__restrict__ probs,
                                                                const uint8_t *__restrict__ moves, int n_valid,
                                                                float *__restrict__ ws) {
    __shared__ prior_sums_t lds[256];
    const int b = blockIdx.x * 256 + threadIdx.x;
    prior_sums_t s[1] = {{0.f, 0.f, 0, 0}};
    const uint32_t mask = b < n_valid ? (uint32_t)moves[b] & ((1u << A) - 1u) : 0u;
    if (mask != 0u) {
        const prior_row_t<A> r = prior_row<A>(probs + (size_t)b * A, mask);
        s[0].l = -cat_log(r.rest < CAT_EPS ? 1.0f - CAT_EPS : r.m);            // 1 - eps passes the clamp as it is
        s[0].m = r.m;
        s[0].lab = 1;
        s[0].agree = (int)((mask >> r.top) & 1u);
    }
    block_sum(s, lds);
    if (threadIdx.x == 0) {
        ws[4 * blockIdx.x] = s[0].l; ws[4 * blockIdx.x + 1] = s[0].m;
        ws[4 * blockIdx.x + 2] = __int_as_float(s[0].lab); ws[4 * blockIdx.x + 3] = __int_as_float(s[0].agree);
    }
}

// pass 2: every workgroup adds the partial counts in block order (the same value everywhere), writes its rows of the
// gradient, and workgroup 0 writes the means and the counts.
template <int A>
__global__ __launch_bounds__(256) void ppo_prior_grad_kernel(const float *__restrict__ probs, const uint8_t *__restrict__ moves,
                                                             int B, int n_valid, float coef, const float *__restrict__ ws,
                                                             int nblocks, float *__restrict__ out, int32_t *__restrict__ counts,
                                                             float *__restrict__ grad_probs) {
    __shared__ int s_lab;
    if (threadIdx.x == 0) {
        int lab = 0, agree = 0;
        float l = 0.f, m = 0.f;
        for (int k = 0; k < nblocks; ++k) {                                 // fixed order
            l += ws[4 * k]; m += ws[4 * k + 1];
            lab += __float_as_int(ws[4 * k + 2]); agree += __float_as_int(ws[4 * k + 3]);
        }
        s_lab = lab;
        if (blockIdx.x == 0) {
            out[0] = lab > 0 ? coef * (l / (float)lab) : 0.f;
            out[1] = lab > 0 ? m / (float)lab : 0.f;
            counts[0] = lab; counts[1] = agree;
        }
    }
    __syncthreads();
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= B) return;
    float g[A];
#pragma unroll
    for (int k = 0; k < A; ++k) g[k] = 0.f;
    const uint32_t mask = b < n_valid ? (uint32_t)moves[b] & ((1u << A) - 1u) : 0u;
    if (mask != 0u) {
        const prior_row_t<A> r = prior_row<A>(probs + (size_t)b * A, mask);
        if (r.m >= CAT_EPS && r.rest >= CAT_EPS) {                          // inside the clamp: the gradient passes
            const float scale = coef / (float)s_lab, in = 1.0f - 1.0f / r.m;
#pragma unroll
            for (int k = 0; k < A; ++k) g[k] = (((mask >> k) & 1u) ? in : 1.0f) / r.S * scale;
        }
    }
#pragma unroll
    for (int k = 0; k < A; ++k) grad_probs[(size_t)b * A + k] = g[k];
}

// ------------------------------------------------------------------ stack gather / age scan
// frame element -> fp32 policy input: identity for float frames, 4-entry LUT for uint8 code frames (TW_F_MATRIX_CODE)
__device__ __forceinline__ float frame_value(float v) { return v; }
__device__ __forceinline__ float frame_value(uint8_t c) {
    return c == 0 ? 0.9f : (c == 1 ? -0.9f : (c == 2 ? -0.5f : 0.3f));
}

// One wavefront per SAMPLE (block = 4 waves = 4 samples): the three index words are fetched once, then the loads of
// all four stack slots (4 x 289 elements) are issued before any of them is stored -- 4.6 KB in flight per wave instead
// of the 1.2 KB of the wave-per-(sample, slot) version, which sat at 0.42 of the HBM peak on its dependent
// index -> row round trips.
template <typename FT>
__global__ __launch_bounds__(256) void ppo_gather_stack_kernel(const FT *__restrict__ frames, int frame_pitch,
                                                               const float *__restrict__ pos_frames, int N,
                                                               const int32_t *__restrict__ k_idx,
                                                               const int32_t *__restrict__ n_idx,
                                                               const int32_t *__restrict__ age,
                                                               const float *__restrict__ init_frame,
                                                               const float *__restrict__ init_pos, int B,
                                                               float *__restrict__ out, float *__restrict__ pos_out) {
    const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= B) return;
    const int lane = threadIdx.x & 63;
    const int k = k_idx[b], n = n_idx[b], ag = age[b];
    constexpr int PER = (TW_CELLS + 63) / 64;                  // 5 elements per lane and slot
    float v[4][PER];
    float ps[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int back = 3 - j;
        const bool use_init = ag - back <= 0;
        const size_t row = ((size_t)(k - back) * N + n);
        const FT *src = frames + row * frame_pitch;
#pragma unroll
        for (int i = 0; i < PER; ++i) {
            const int c = lane + 64 * i;
            v[j][i] = c < TW_CELLS ? (use_init ? init_frame[c] : frame_value(src[c])) : 0.f;
        }
        if (pos_out && lane < 2) ps[j] = use_init ? init_pos[lane] : pos_frames[row * 2 + lane];
    }
    float *dst = out + (size_t)b * 4 * TW_CELLS;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
#pragma unroll
        for (int i = 0; i < PER; ++i) {
            const int c = lane + 64 * i;
            if (c < TW_CELLS) dst[j * TW_CELLS + c] = v[j][i];
        }
        if (pos_out && lane < 2) pos_out[((size_t)b * 4 + j) * 2 + lane] = ps[j];
    }
}

// ------------------------------------------------------------------ hindsight relabelling (HER)
// Buffer_gridworld.her_func (soa/env_buffer.py:101-143) over a time-major rollout.  The reference copies
// episode prefixes into its ring buffer; here a relabelled transition is only an index record
// (t, n, goal', reward', done'): the frames / positions / action / old log-prob are those of (t, n).
// One wavefront per env walks its episodes in time order; an episode (<= 64 steps) sits one step per lane.
constexpr int HER_MAX_LEN = 64;

// np.unique(axis=0) of an episode that sits one record per lane, (py, px) = lane's achieved (y, x), L <= 64 records:
// first = this lane holds the first occurrence of its (y, x), rank = its place among the first occurrences ordered
// lexicographically by (y, x) -- the unit of `choices`; returns the mask of first occurrences.  Float compares, so
// +0.0 and -0.0 are one position.  Window records (skip = 4, env_buffer.py:145-280) only offer the states after steps
// skip, skip + 1, ...  Every lane of the wavefront must call this.
__device__ __forceinline__ unsigned long long her_first_visits(float py, float px, int lane, int L, int skip, bool &first,
                                                               int &rank) {
    first = lane < L && lane >= skip;
    for (int j = skip; j < L; ++j) {
        const float qy = __shfl(py, j), qx = __shfl(px, j);
        if (j < lane && qy == py && qx == px) first = false;
    }
    const unsigned long long fm = __ballot(first);
    rank = 0;
    for (int j = 0; j < L; ++j) {
        const float qy = __shfl(py, j), qx = __shfl(px, j);
        if (((fm >> j) & 1ull) && (qy < py || (qy == py && qx < px))) ++rank;
    }
    return fm;
}

__global__ __launch_bounds__(64) void ppo_her_kernel(const float *__restrict__ pos, const uint8_t *__restrict__ terminated,
                                                     const uint8_t *__restrict__ truncated,
                                                     const int32_t *__restrict__ age0, const float *__restrict__ reward,
                                                     const int32_t *__restrict__ choices, uint32_t k0, uint32_t k1,
                                                     uint32_t env_id0, uint32_t step0, int T, int N, int max_goals, int skip,
                                                     const int64_t *__restrict__ offsets, int32_t *__restrict__ counts,
                                                     int32_t *__restrict__ out_t, int32_t *__restrict__ out_n,
                                                     float *__restrict__ out_goal, float *__restrict__ out_reward,
                                                     uint8_t *__restrict__ out_done) {
    const int n = blockIdx.x;
    const int lane = threadIdx.x;
    if (n >= N) return;
    const bool emit = offsets != nullptr;
    int64_t base = emit ? offsets[n] : 0;
    int total = 0;
    int start = age0[n] == 0 ? 0 : -1;               // an episode already running at t = 0 is not relabelled
    for (int c0 = 0; c0 < T; c0 += 64) {
        const int tl = c0 + lane;
        const bool d = tl < T && done_at(terminated, truncated, (size_t)tl * N + n) != 0;
        unsigned long long dm = __ballot(d);
        while (dm) {
            const int t1 = c0 + __builtin_ctzll(dm);
            dm &= dm - 1;
            const int s0 = start;
            start = t1 + 1;
            if (s0 < 0) continue;
            const int L = t1 - s0 + 1;
            if (L > HER_MAX_LEN) continue;
            // lane i = record i of the episode: achieved (y, x) after step s0 + i
            const bool in = lane < L;
            const size_t row = (size_t)(s0 + (in ? lane : 0)) * N + n;
            const float py = pos[row * 2], px = pos[row * 2 + 1];
            bool first;
            int rank;
            const int U = __popcll(her_first_visits(py, px, lane, L, skip, first, rank));
            const int k = max_goals < U ? max_goals : U;
            // Fisher-Yates over the U unique entries when no explicit picks are supplied (lane j holds perm[j])
            int perm = lane;
            if (!choices) {
                uint32_t w0 = env_id0 + (uint32_t)n, w1 = step0 + (uint32_t)t1, w2 = 0, w3 = 0x54574F48u;   // 'TWOH'
                philox4x32_10(k0, k1, w0, w1, w2, w3);
                const uint32_t w[4] = {w0, w1, w2, w3};
                for (int j = 0; j < k && j < 4; ++j) {
                    const int sidx = j + (int)(w[j] % (uint32_t)(U - j));
                    const int pj = __shfl(perm, j), ps = __shfl(perm, sidx);
                    if (lane == j) perm = ps;
                    else if (lane == sidx) perm = pj;
                }
            }
            for (int j = 0; j < k; ++j) {
                const int pick = choices ? choices[((size_t)t1 * N + n) * 4 + j] : __shfl(perm, j);
                if (pick < 0 || pick >= U) continue;
                const unsigned long long hit = __ballot(first && rank == pick);
                if (!hit) continue;
                const int idx = __builtin_ctzll(hit);
                if (idx == skip) continue;                               // env_buffer.py:119 / :163 `if 0 < index < cap`
                if (emit && lane <= idx) {
                    const int64_t o = base + lane;
                    out_t[o] = s0 + lane;
                    out_n[o] = n;
                    out_goal[o * 2] = __shfl(py, idx);
                    out_goal[o * 2 + 1] = __shfl(px, idx);
                    out_reward[o] = lane == idx ? 0.9f : reward[row];
                    out_done[o] = lane == idx ? 1 : 0;
                }
                base += idx + 1;
                total += idx + 1;
            }
        }
    }
    if (lane == 0 && counts) counts[n] = total;
}

// Which first visits become goals, by rule: the picks ppo_her_kernel reads as `choices`.  The same walk over the same
// episodes; the candidates are the first visits but the one at record `skip`, which the relabelling never uses
// (`0 < index`).  The smallest (key, Philox word, rank) comes first; a lane finds its place by counting the candidates
// that come before it, one broadcast per candidate.  The tallies stay in registers until the env is walked.
__global__ __launch_bounds__(64) void ppo_her_select_kernel(const float *__restrict__ pos, const uint8_t *__restrict__ terminated,
                                                            const uint8_t *__restrict__ truncated,
                                                            const int32_t *__restrict__ age0, int T, int N, int max_goals,
                                                            int skip, int rule, const uint16_t *__restrict__ key16,
                                                            const int64_t *__restrict__ table, int width, int height,
                                                            uint32_t k0, uint32_t k1, uint32_t env_id0, uint32_t step0,
                                                            int32_t *__restrict__ choices,
                                                            unsigned long long *__restrict__ stats) {
    const int n = blockIdx.x;
    const int lane = threadIdx.x;
    if (n >= N) return;
    long long tally = 0;                             // lane j < 6 carries stats[j] of this env
    long long prefix_sum = 0, key_sum = 0;           // per lane, summed over the lanes at the end
    int unreachable = 0;
    int start = age0[n] == 0 ? 0 : -1;               // an episode already running at t = 0 is not relabelled
    for (int c0 = 0; c0 < T; c0 += 64) {
        const int tl = c0 + lane;
        const bool d = tl < T && done_at(terminated, truncated, (size_t)tl * N + n) != 0;
        unsigned long long dm = __ballot(d);
        while (dm) {
            const int t1 = c0 + __builtin_ctzll(dm);
            dm &= dm - 1;
            const int s0 = start;
            start = t1 + 1;
            if (s0 < 0) continue;
            const int L = t1 - s0 + 1;
            if (L > HER_MAX_LEN) continue;
            const bool in = lane < L;
            const size_t row = (size_t)(s0 + (in ? lane : 0)) * N + n;
            const float py = pos[row * 2], px = pos[row * 2 + 1];
            bool first;
            int rank;
            const unsigned long long fm = her_first_visits(py, px, lane, L, skip, first, rank);
            const bool cand = first && lane != skip;
            const unsigned long long cm = fm & ~(1ull << skip);
            const int C = __popcll(cm);
            long long key = 0;
            uint32_t word = 0;
            if (cand) {
                if (rule == PPO_HER_LATE) key = 63 - lane;
                else if (rule == PPO_HER_KEY16) key = key16[row];
                else key = table[visit_cell(py, px, width, height)];
                uint32_t w1 = step0 + (uint32_t)t1, w2 = (uint32_t)rank, w3 = 0x54574F53u;   // 'TWOS'
                word = env_id0 + (uint32_t)n;
                philox4x32_10(k0, k1, word, w1, w2, w3);
            }
            const unsigned long long tie = ((unsigned long long)word << 32) | (uint32_t)rank;
            int place = 0;
            for (unsigned long long m = cm; m; m &= m - 1) {
                const int j = __builtin_ctzll(m);
                const long long qk = __shfl(key, j);
                const unsigned long long qt = __shfl(tie, j);
                if (qk < key || (qk == key && qt < tie)) ++place;
            }
            const int k = max_goals < C ? max_goals : C;
            int32_t *out = choices + ((size_t)t1 * N + n) * 4;
            const bool picked = cand && place < k;
            if (picked) {
                out[place] = rank;
                prefix_sum += lane + 1;
                if (rule == PPO_HER_KEY16 && key == 0xFFFF) ++unreachable;
                else if (rule != PPO_HER_LATE) key_sum += key;
            }
            if (lane < 4 && lane >= k) out[lane] = -1;
            tally += lane == 0 ? 1 : lane == 1 ? C : lane == 2 ? k : 0;
        }
    }
    if (!stats) return;
    long long unreachable_sum = unreachable;
    for (int off = 32; off > 0; off >>= 1) {
        prefix_sum += __shfl_xor(prefix_sum, off);
        key_sum += __shfl_xor(key_sum, off);
        unreachable_sum += __shfl_xor(unreachable_sum, off);
    }
    if (lane == 3) tally = prefix_sum;
    if (lane == 4) tally = key_sum;
    if (lane == 5) tally = unreachable_sum;
    if (lane < 6 && tally != 0) atomicAdd(&stats[lane], (unsigned long long)tally);
}

__global__ void ppo_age_scan_kernel(const uint8_t *__restrict__ terminated, const uint8_t *__restrict__ truncated,
                                    const int32_t *__restrict__ age0, int T, int N, int32_t *__restrict__ age) {
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N) return;
    int a = age0[n];
    age[n] = a;
    for (int t = 0; t < T; ++t) {
        const size_t i = (size_t)t * N + n;
        a = done_at(terminated, truncated, i) ? 0 : a + 1;
        age[(size_t)(t + 1) * N + n] = a;
    }
}

// ------------------------------------------------------------------ episode accounting
// Per-episode return and length, carried across launches (train_ppo.py:124 `ep_reward += reward`, :136-141).  One lane
// per env over coalesced rows; the float64 additions are one per step in step order, so the bits do not depend on how
// a rollout is cut into launches.  The dependent chain is T adds per lane and costs nothing next to the loads, which
// are issued EP_ROWS rows ahead of it: the rows of batch k + 1 are in flight while batch k is added up and stored.
constexpr int EP_ROWS = 8;

__global__ __launch_bounds__(64) void ppo_episode_scan_kernel(const float *__restrict__ reward,
                                                              const uint8_t *__restrict__ terminated,
                                                              const uint8_t *__restrict__ truncated, int T, int N,
                                                              double *__restrict__ carry_return,
                                                              int32_t *__restrict__ carry_length,
                                                              double *__restrict__ ep_return,
                                                              int32_t *__restrict__ ep_length) {
    const int n = blockIdx.x * 64 + threadIdx.x;
    if (n >= N) return;
    double acc = carry_return[n];
    int len = carry_length[n];
    float r[EP_ROWS], rn[EP_ROWS];
    uint32_t d[EP_ROWS], dn[EP_ROWS];
#pragma unroll
    for (int j = 0; j < EP_ROWS; ++j) {
        const size_t i = (size_t)j * N + n;
        r[j] = j < T ? reward[i] : 0.f;
        d[j] = j < T ? (uint32_t)(terminated[i] | truncated[i]) : 0u;      // not done_at: DESIGN.md 6.20
    }
    for (int t0 = 0; t0 < T; t0 += EP_ROWS) {
#pragma unroll
        for (int j = 0; j < EP_ROWS; ++j) {                         // next batch: loads only, nothing waits on them yet
            const int t = t0 + EP_ROWS + j;
            const size_t i = (size_t)t * N + n;
            rn[j] = t < T ? reward[i] : 0.f;
            dn[j] = t < T ? (uint32_t)(terminated[i] | truncated[i]) : 0u;
        }
#pragma unroll
        for (int j = 0; j < EP_ROWS; ++j) {
            const int t = t0 + j;
            if (t < T) {
                const size_t i = (size_t)t * N + n;
                acc += (double)r[j];
                len += 1;
                if (ep_return) ep_return[i] = acc;
                if (ep_length) ep_length[i] = len;
                if (d[j]) { acc = 0.0; len = 0; }
            }
        }
#pragma unroll
        for (int j = 0; j < EP_ROWS; ++j) { r[j] = rn[j]; d[j] = dn[j]; }
    }
    carry_return[n] = acc;
    carry_length[n] = len;
}

// What one rollout's finished episodes looked like, and the reference's running score folded over them in row-major
// (t, then n) order (train_ppo.py:140 `running_score = running_score * 0.99 + ep_reward * 0.01`).  A partial result is
// EP_NV doubles (counts are integers far below 2^53, hence exact):
//   0 a, 1 b        the fold of a run of steps as ONE affine map score -> score * a + b; a step that is not done is the
//                   identity (1, 0); runs compose left to right: (a1, b1) then (a2, b2) = (a1 a2, b1 a2 + b2)
//   2 episodes, 3 successes, 4 truncated-only, 5 sum return, 6 min return, 7 max return, 8 sum length, 9 max length
//   10..16 action histogram, 17..22 reward histogram
// Every thread walks a contiguous run of the row-major index range, lanes and waves are combined in index order, each
// workgroup writes one partial, and one wavefront combines the partials in block order: a fixed grid and a fixed
// order for a given (T, N), hence deterministic.
constexpr int EP_NV = 24, EP_ACT = 10, EP_REW = 17, EP_MAX_ACTIONS = 7;
constexpr int EP_BLOCK_ELEMS = 2048, EP_MAX_BLOCKS = 256;

__device__ __forceinline__ void ep_identity(double (&v)[EP_NV]) {
#pragma unroll
    for (int k = 0; k < EP_NV; ++k) v[k] = 0.0;
    v[0] = 1.0;
    v[6] = (double)INFINITY;
    v[7] = -(double)INFINITY;
}

// v <- v followed by w
__device__ __forceinline__ void ep_combine(double (&v)[EP_NV], const double (&w)[EP_NV]) {
    v[1] = v[1] * w[0] + w[1];
    v[0] = v[0] * w[0];
    v[6] = fmin(v[6], w[6]);
    v[7] = fmax(v[7], w[7]);
    v[9] = fmax(v[9], w[9]);
#pragma unroll
    for (int k = 2; k < EP_NV; ++k)
        if (k != 6 && k != 7 && k != 9) v[k] += w[k];
}

// Ordered reduction over the 64 lanes of a wavefront: after step s a lane whose index is a multiple of 2s holds the
// combination of lanes [lane, lane + 2s) in lane order; lane 0 ends with all 64 (the other lanes hold don't-cares).
__device__ __forceinline__ void ep_wave_reduce(double (&v)[EP_NV]) {
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) {
        double w[EP_NV];
#pragma unroll
        for (int k = 0; k < EP_NV; ++k) w[k] = __shfl_down(v[k], s, 64);
        ep_combine(v, w);
    }
}

__device__ __forceinline__ int ep_reward_bucket(float r) {
    return r == -0.01f ? 0 : (r == -0.1f ? 1 : (r == -0.9f ? 2 : (r == 0.2f ? 3 : (r == 0.9f ? 4 : 5))));
}

__global__ __launch_bounds__(256) void ppo_episode_partial_kernel(const double *__restrict__ ep_return,
                                                                  const int32_t *__restrict__ ep_length,
                                                                  const uint8_t *__restrict__ terminated,
                                                                  const uint8_t *__restrict__ truncated,
                                                                  const float *__restrict__ reward,
                                                                  const int32_t *__restrict__ action, int64_t M,
                                                                  int64_t per_block, int per_thread, double keep,
                                                                  double gain, double *__restrict__ ws) {
    __shared__ double sh[4][EP_NV];
    const int64_t block_lo = (int64_t)blockIdx.x * per_block;
    const int64_t block_hi = block_lo + per_block < M ? block_lo + per_block : M;
    int64_t lo = block_lo + (int64_t)threadIdx.x * per_thread;
    int64_t hi = lo + per_thread;
    if (hi > block_hi) hi = block_hi;
    double a = 1.0, b = 0.0, sum_r = 0.0, min_r = (double)INFINITY, max_r = -(double)INFINITY;
    long long sum_len = 0;
    int episodes = 0, successes = 0, max_len = 0;
    int ah[EP_MAX_ACTIONS], rh[6];
#pragma unroll
    for (int k = 0; k < EP_MAX_ACTIONS; ++k) ah[k] = 0;
#pragma unroll
    for (int k = 0; k < 6; ++k) rh[k] = 0;
    for (int64_t i0 = lo; i0 < hi; i0 += EP_ROWS) {
        float r[EP_ROWS];
        uint32_t te[EP_ROWS], tr[EP_ROWS];
        int ac[EP_ROWS];
#pragma unroll
        for (int j = 0; j < EP_ROWS; ++j) {                         // the batch's loads first, the fold after them
            const int64_t i = i0 + j;
            const bool in = i < hi;
            r[j] = in ? reward[i] : 0.f;
            te[j] = in ? (uint32_t)terminated[i] : 0u;
            tr[j] = in ? (uint32_t)truncated[i] : 0u;
            ac[j] = (in && action) ? action[i] : -1;
        }
#pragma unroll
        for (int j = 0; j < EP_ROWS; ++j) {
            const int64_t i = i0 + j;
            if (i < hi) {
                const int bucket = ep_reward_bucket(r[j]);
#pragma unroll
                for (int k = 0; k < 6; ++k) rh[k] += (bucket == k);
#pragma unroll
                for (int k = 0; k < EP_MAX_ACTIONS; ++k) ah[k] += (ac[j] == k);
                if (te[j] | tr[j]) {                                 // an episode ends here: its return and length
                    const double R = ep_return[i];
                    const int L = ep_length[i];
                    b = b * keep + R * gain;
                    a = a * keep;
                    episodes += 1;
                    successes += te[j] ? 1 : 0;
                    sum_r += R;
                    min_r = fmin(min_r, R);
                    max_r = fmax(max_r, R);
                    sum_len += L;
                    max_len = L > max_len ? L : max_len;
                }
            }
        }
    }
    double v[EP_NV];
    ep_identity(v);
    v[0] = a; v[1] = b;
    v[2] = (double)episodes; v[3] = (double)successes; v[4] = (double)(episodes - successes);
    v[5] = sum_r; v[6] = min_r; v[7] = max_r; v[8] = (double)sum_len; v[9] = (double)max_len;
#pragma unroll
    for (int k = 0; k < EP_MAX_ACTIONS; ++k) v[EP_ACT + k] = (double)ah[k];
#pragma unroll
    for (int k = 0; k < 6; ++k) v[EP_REW + k] = (double)rh[k];
    ep_wave_reduce(v);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int k = 0; k < EP_NV; ++k) sh[wave][k] = v[k];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; ++w) {                                // waves in index order
            double o[EP_NV];
#pragma unroll
            for (int k = 0; k < EP_NV; ++k) o[k] = sh[w][k];
            ep_combine(v, o);
        }
#pragma unroll
        for (int k = 0; k < EP_NV; ++k) ws[(size_t)blockIdx.x * EP_NV + k] = v[k];
    }
}

__global__ __launch_bounds__(64) void ppo_episode_finalize_kernel(const double *__restrict__ ws, int nblocks, int A,
                                                                  double *__restrict__ score,
                                                                  double *__restrict__ summary,
                                                                  int64_t *__restrict__ action_hist,
                                                                  int64_t *__restrict__ reward_hist) {
    const int lane = threadIdx.x;
    const int per_lane = (nblocks + 63) / 64;                        // nblocks <= EP_MAX_BLOCKS: at most 4 each
    double v[EP_NV];
    ep_identity(v);
    for (int j = 0; j < per_lane; ++j) {                             // lane l: blocks [l * per_lane, (l + 1) * per_lane)
        const int blk = lane * per_lane + j;
        if (blk < nblocks) {
            double o[EP_NV];
#pragma unroll
            for (int k = 0; k < EP_NV; ++k) o[k] = ws[(size_t)blk * EP_NV + k];
            ep_combine(v, o);
        }
    }
    ep_wave_reduce(v);
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < 8; ++k) summary[k] = v[2 + k];
#pragma unroll
        for (int k = 0; k < EP_MAX_ACTIONS; ++k)
            if (action_hist && k < A) action_hist[k] = (int64_t)v[EP_ACT + k];
#pragma unroll
        for (int k = 0; k < 6; ++k) reward_hist[k] = (int64_t)v[EP_REW + k];
        if (score && v[2] > 0.0) *score = *score * v[0] + v[1];      // no finished episode: not written at all
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// World-model decoder, inference only (Net_Decoder, all_net.py:100-137): latent float[64][4][4] per frame ->
//   ConvTranspose2d(64->16, k2, s2) + ReLU  -> a1[8][8][16]
//   ConvTranspose2d(16->16, k5, s4) + ReLU  -> a2[33][33][16]
//   ConvTranspose2d(16->1,  k4, s2)         -> 68x68,  AvgPool2d(4) -> 17x17
// The last layer and the pooling are both linear, so together they are ONE 3x3 / stride-2 / pad-1 convolution of a2
// with pre-summed taps (kfold, see ppo_decoder_frames in twoarmy_ppo.h): the 68x68 image never exists.  One workgroup
// walks frames with a grid stride; weights stay in LDS, a frame's activations never leave LDS (120 KB per workgroup).
constexpr int DEC_A2 = 33 * 33 * 16;

__global__ __launch_bounds__(256) void ppo_decoder_frames_kernel(const float *__restrict__ z, int n_frames,
                                                                 const float *__restrict__ w1, const float *__restrict__ b1,
                                                                 const float *__restrict__ w2, const float *__restrict__ b2,
                                                                 const float *__restrict__ kfold, float b3,
                                                                 float *__restrict__ frames) {
    __shared__ __attribute__((aligned(16))) float W2s[16 * 25 * 16];      // [ci][tap][co]
    __shared__ __attribute__((aligned(16))) float W1s[64 * 4 * 16];       // [ci][ky*2+kx][co]
    __shared__ __attribute__((aligned(16))) float Ks[9 * 16];             // [u*3+v][c]
    __shared__ __attribute__((aligned(16))) float B1s[16], B2s[16];
    __shared__ __attribute__((aligned(16))) float zs[64 * 16];            // [ci][iy*4+ix]
    __shared__ __attribute__((aligned(16))) float a1s[64 * 16];           // [oy*8+ox][c]
    __shared__ __attribute__((aligned(16))) float a2s[DEC_A2];            // [oy*33+ox][c]
    const int tid = threadIdx.x;
    // ConvTranspose2d weights are [C_in][C_out][kH][kW]
    for (int i = tid; i < 16 * 16 * 25; i += 256) {
        const int ci = i / 400, r = i - ci * 400, co = r / 25, tap = r - co * 25;
        W2s[(ci * 25 + tap) * 16 + co] = w2[i];
    }
    for (int i = tid; i < 64 * 16 * 4; i += 256) {
        const int ci = i >> 6, r = i & 63, co = r >> 2, k = r & 3;
        W1s[(ci * 4 + k) * 16 + co] = w1[i];
    }
    if (tid < 144) { const int c = tid / 9, t = tid - c * 9; Ks[t * 16 + c] = kfold[tid]; }     // kfold is [c][u][v]
    if (tid < 16) { B1s[tid] = b1[tid]; B2s[tid] = b2[tid]; }
    for (int f = blockIdx.x; f < n_frames; f += gridDim.x) {
        __syncthreads();                                   // weights loaded / previous frame's stage 3 done with a2s
        for (int i = tid; i < 1024; i += 256) zs[i] = z[(size_t)f * 1024 + i];
        __syncthreads();
        // ---- stage 1: every output pixel has exactly one source pixel (k2, s2)
        for (int o = tid; o < 1024; o += 256) {
            const int co = o & 15, pix = o >> 4, oy = pix >> 3, ox = pix & 7;
            const int src = (oy >> 1) * 4 + (ox >> 1), k = (oy & 1) * 2 + (ox & 1);
            float acc = B1s[co];
#pragma unroll 8
            for (int ci = 0; ci < 64; ++ci) acc = fmaf(zs[ci * 16 + src], W1s[(ci * 4 + k) * 16 + co], acc);
            a1s[pix * 16 + co] = fmaxf(acc, 0.0f);
        }
        __syncthreads();
        // ---- stage 2: output row oy receives input row oy>>2 through tap row oy&3 and, where oy is a multiple of 4,
        //      input row (oy>>2)-1 through tap row 4 (k5, s4: neighbouring patches overlap by one line); columns alike
        for (int item = tid; item < 33 * 33 * 4; item += 256) {
            const int q = item & 3, pix = item >> 2, oy = pix / 33, ox = pix - oy * 33;
            float4 acc = *reinterpret_cast<const float4 *>(&B2s[q * 4]);
            const int iy0 = oy >> 2, ky0 = oy & 3, ix0 = ox >> 2, kx0 = ox & 3;
#pragma unroll
            for (int ry = 0; ry < 2; ++ry) {
                const int iy = ry ? iy0 - 1 : iy0, ky = ry ? 4 : ky0;
                if (ry ? (ky0 != 0 || iy0 == 0) : (iy0 > 7)) continue;
#pragma unroll
                for (int rx = 0; rx < 2; ++rx) {
                    const int ix = rx ? ix0 - 1 : ix0, kx = rx ? 4 : kx0;
                    if (rx ? (kx0 != 0 || ix0 == 0) : (ix0 > 7)) continue;
                    const float *a = &a1s[(iy * 8 + ix) * 16];
                    const float *w = &W2s[(ky * 5 + kx) * 16 + q * 4];
#pragma unroll
                    for (int ci = 0; ci < 16; ++ci)
                        acc = fma4(a[ci], *reinterpret_cast<const float4 *>(w + ci * 400), acc);
                }
            }
            *reinterpret_cast<float4 *>(&a2s[pix * 16 + q * 4]) = relu4(acc);
        }
        __syncthreads();
        // ---- stage 3: last transposed conv + 4x4 average pooling = 3x3 / stride 2 / pad 1 over a2
        for (int o = tid; o < 289; o += 256) {
            const int y = o / 17, x = o - y * 17;
            float acc = b3;
#pragma unroll
            for (int u = 0; u < 3; ++u) {
                const int iy = 2 * y + u - 1;
                if ((unsigned)iy > 32u) continue;
#pragma unroll
                for (int v = 0; v < 3; ++v) {
                    const int ix = 2 * x + v - 1;
                    if ((unsigned)ix > 32u) continue;
                    const float4 *a = reinterpret_cast<const float4 *>(&a2s[(iy * 33 + ix) * 16]);
                    const float4 *k = reinterpret_cast<const float4 *>(&Ks[(u * 3 + v) * 16]);
#pragma unroll
                    for (int c = 0; c < 4; ++c) {
                        const float4 av = a[c], kv = k[c];
                        acc = fmaf(av.x, kv.x, acc); acc = fmaf(av.y, kv.y, acc);
                        acc = fmaf(av.z, kv.z, acc); acc = fmaf(av.w, kv.w, acc);
                    }
                }
            }
            frames[(size_t)f * 289 + o] = acc;
        }
    }
}

// LSTM cell, pointwise part (torch gate order i, f, g, o): c' = sigmoid(f) c + sigmoid(i) tanh(g), h' = sigmoid(o) tanh(c').
// The pre-activations are the sum of up to three terms, added here instead of in GEMM epilogues / copy kernels:
// gates_a float[B][4H] (a GEMM result), gates_b (optional, rows ldb floats apart: the slice of one time step out of
// the input projections of all known steps) and bias (optional, float[4H]).  One pass instead of eight elementwise
// launches plus the strided copy torch.addmm makes of a non-contiguous addend.
__global__ __launch_bounds__(256) void ppo_lstm_cell_kernel(const float4 *__restrict__ ga, const float4 *__restrict__ gb,
                                                            long long ldb4, const float4 *__restrict__ bias,
                                                            float4 *__restrict__ c, float4 *__restrict__ h, int B, int H4) {
    const int i = blockIdx.x * 256 + threadIdx.x;                 // one float4 of one row's hidden vector
    if (i >= B * H4) return;
    const int b = i / H4, j = i - b * H4;
    float4 gi = make_float4(0.f, 0.f, 0.f, 0.f), gf = gi, gg = gi, go = gi;
    if (ga) {
        const float4 *g = ga + (size_t)b * 4 * H4;
        gi = g[j]; gf = g[H4 + j]; gg = g[2 * H4 + j]; go = g[3 * H4 + j];
    }
    // its own add4, not the shared one, which costs 6 VGPRs and 0.1 us here
    auto add4 = [](float4 &a, const float4 &v) { a.x += v.x; a.y += v.y; a.z += v.z; a.w += v.w; };
    if (gb) {
        const float4 *q = gb + (size_t)b * ldb4;
        add4(gi, q[j]); add4(gf, q[H4 + j]); add4(gg, q[2 * H4 + j]); add4(go, q[3 * H4 + j]);
    }
    if (bias) { add4(gi, bias[j]); add4(gf, bias[H4 + j]); add4(gg, bias[2 * H4 + j]); add4(go, bias[3 * H4 + j]); }
    float4 cv = c[i], hv;
    auto sig = [](float x) { return 1.0f / (1.0f + __expf(-x)); };
#define LSTM_LANE(m)                                                                                                      \
    cv.m = sig(gf.m) * cv.m + sig(gi.m) * tanhf(gg.m);                                                                   \
    hv.m = sig(go.m) * tanhf(cv.m);
    LSTM_LANE(x) LSTM_LANE(y) LSTM_LANE(z) LSTM_LANE(w)
#undef LSTM_LANE
    c[i] = cv;
    h[i] = hv;
}

// ------------------------------------------------------------------ host: argument rules, grids, dispatch
template <typename... P> bool all_set(const P *...p) { return (... && (p != nullptr)); }
template <typename... P> bool aligned16(const P *...p) { return ((... | (uintptr_t)p) & 15u) == 0; }     // NULL counts as aligned
// every pointer on the alignment of its own element type (float / int32: 4 bytes, double / int64: 8); NULL counts as aligned
template <typename... P> bool aligned_natural(const P *...p) { return (... && ((uintptr_t)p % alignof(P) == 0)); }
bool ep_count_ok(int64_t M) { return M < ((int64_t)1 << 40); }      // T * N of the episode entries: a thread's run stays an int
bool gr_count_ok(int64_t H) { return H > 0 && H < ((int64_t)1 << 40); }    // the record entries: grids and workspace stay ints
// Levels of the scan tree of ppo_gae_runs: n[0] = H records, n[l + 1] = ceil(n[l] / GR_BLOCK) composites for as long as
// level l has more maps than one workgroup takes.  Returns the number of levels (>= 1).
int gr_levels(int64_t H, int64_t (&n)[GR_MAX_LEVELS]) {
    int levels = 1;
    n[0] = H;
    while (n[levels - 1] > GR_BLOCK) { n[levels] = (n[levels - 1] + GR_BLOCK - 1) / GR_BLOCK; ++levels; }
    return levels;
}
int blocks(int64_t n, int per) { return (int)((n + per - 1) / per); }
int blocks_capped(int64_t n, int per, int cap) { return (int)((n + per - 1) / per < cap ? (n + per - 1) / per : cap); }
int ep_summary_blocks(int64_t M) { return blocks_capped(M, EP_BLOCK_ELEMS, EP_MAX_BLOCKS); }
float4 *f4(float *p) { return reinterpret_cast<float4 *>(p); }
const float4 *f4(const float *p) { return reinterpret_cast<const float4 *>(p); }
template <int V> using int_c = std::integral_constant<int, V>;

// The action counts the templated kernels are built for, stated once: the rule, and runtime A -> fn(int_c<A>).
#define PPO_ACTION_COUNTS(X) X(5) X(2) X(3) X(4) X(7)
bool ppo_actions_ok(int A) {
#define PPO_IS(V) if (A == V) return true;
    PPO_ACTION_COUNTS(PPO_IS)
#undef PPO_IS
    return false;
}
template <typename Fn> void ppo_with_actions(int A, Fn &&fn) {      // A has passed ppo_actions_ok
    switch (A) {
#define PPO_CASE(V) case V: fn(int_c<V>{}); break;
    PPO_ACTION_COUNTS(PPO_CASE)
#undef PPO_CASE
    }
}

template <typename FT>
int gather_stack(const char *what, const FT *frames, int frame_pitch, const float *pos_frames, int N, const int32_t *k_idx,
                 const int32_t *n_idx, const int32_t *age, const float *init_frame, const float *init_pos, int B,
                 float *out, float *pos_out, void *stream) {
    if (!all_set(frames, k_idx, n_idx, age, init_frame, out) || B <= 0 || frame_pitch < TW_CELLS) return TW_E_ARG;
    if (pos_out && !all_set(pos_frames, init_pos)) return TW_E_ARG;
    hipLaunchKernelGGL(ppo_gather_stack_kernel<FT>, dim3(blocks(B, 4)), dim3(256), 0, (hipStream_t)stream, frames, frame_pitch,
                       pos_frames, N, k_idx, n_idx, age, init_frame, init_pos, B, out, pos_out);
    return tw_launched(what);
}

}  // namespace

extern "C" {

int ppo_sample(const float *probs, int B, int A, const float *uniforms, uint64_t seed, uint64_t offset,
               int32_t *action, float *logp, void *stream) {
    return ppo_sample_dev(probs, B, A, uniforms, seed, offset, nullptr, action, logp, stream);
}

int ppo_sample_dev(const float *probs, int B, int A, const float *uniforms, uint64_t seed, uint64_t offset,
                   const uint64_t *offset_dev, int32_t *action, float *logp, void *stream) {
    if (!all_set(probs, action, logp) || B <= 0 || !ppo_actions_ok(A)) return TW_E_ARG;
    const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
    ppo_with_actions(A, [&](auto a) {
        hipLaunchKernelGGL(ppo_sample_kernel<decltype(a)::value>, dim3(blocks(B, 256)), dim3(256), 0, (hipStream_t)stream,
                           probs, B, uniforms, k0, k1, offset, offset_dev, action, logp);
    });
    return tw_launched(__func__);
}

int ppo_gae(const float *reward, const float *value, const float *next_value, const uint8_t *done, float gamma,
            float lambda, int use_done_mask, int T, int N, float *adv, float *target, float *ret, void *stream) {
    if (!all_set(reward, value, next_value) || T <= 0 || N <= 0 || (use_done_mask && !done)) return TW_E_ARG;
    auto launch = [&](auto gn) {                             // envs per workgroup
        hipLaunchKernelGGL(ppo_gae_kernel<decltype(gn)::value>, dim3(blocks(N, decltype(gn)::value)), dim3(256), 0,
                           (hipStream_t)stream, reward, value, next_value, done, gamma, lambda, use_done_mask, T, N, adv,
                           target, ret);
    };
    if (N >= 16384) launch(int_c<64>{});
    else launch(int_c<16>{});
    return tw_launched(__func__);
}

int ppo_run_ends(const int32_t *t, const int32_t *n, const float *goal, const uint8_t *done, int64_t H, uint8_t *run_end,
                 int32_t *broken, void *stream) {
    if (!all_set(t, n, goal, done, run_end) || !gr_count_ok(H)) return TW_E_ARG;
    hipLaunchKernelGGL(ppo_run_ends_kernel, dim3(blocks(H, 1024)), dim3(256), 0, (hipStream_t)stream, t, n, goal,
                       done, H, run_end, broken);
    return tw_launched(__func__);
}

int ppo_gae_runs_workspace(int64_t H) {
    if (!gr_count_ok(H)) return TW_E_ARG;
    int64_t n[GR_MAX_LEVELS];
    const int levels = gr_levels(H, n);
    int64_t floats = 0;
    for (int l = 1; l < levels; ++l) floats += 2 * n[l];
    return (int)(floats > 2 ? floats : 2);
}

int ppo_gae_runs(const float *reward, const float *value, const float *next_value, const uint8_t *done,
                 const uint8_t *run_end, float gamma, float lambda, int use_done_mask, int64_t H, float *adv, float *target,
                 float *ret, float *workspace, void *stream) {
    if (!all_set(reward, value, next_value, run_end, workspace) || !gr_count_ok(H) || (use_done_mask && !done))
        return TW_E_ARG;
    hipStream_t st = (hipStream_t)stream;
    int64_t n[GR_MAX_LEVELS];
    const int levels = gr_levels(H, n);
    float *lc[GR_MAX_LEVELS] = {}, *ld[GR_MAX_LEVELS] = {};      // level l >= 1: c[n_l] then d[n_l]
    for (int l = 1; l < levels; ++l) {
        lc[l] = l == 1 ? workspace : ld[l - 1] + n[l - 1];
        ld[l] = lc[l] + n[l];
    }
    const gr_records rec{reward, value, next_value, done, run_end, gamma, lambda, use_done_mask, adv, target, ret};
    for (int l = 0; l + 1 < levels; ++l) {                       // up: the composites of every level but the top
        if (l == 0)
            hipLaunchKernelGGL(ppo_gae_runs_reduce_kernel<gr_records>, dim3((unsigned)n[1]), dim3(256), 0, st, rec, H, lc[1],
                               ld[1]);
        else
            hipLaunchKernelGGL(ppo_gae_runs_reduce_kernel<gr_composites>, dim3((unsigned)n[l + 1]), dim3(256), 0, st,
                               gr_composites{lc[l], ld[l]}, n[l], lc[l + 1], ld[l + 1]);
    }
    for (int l = levels - 1; l >= 0; --l) {                      // down: the top from x = 0, the rest from the level above
        const float *carry = l + 1 < levels ? ld[l + 1] : nullptr;
        const int64_t n_carry = l + 1 < levels ? n[l + 1] : 0;
        const dim3 grid((unsigned)blocks(n[l], GR_BLOCK));
        if (l == 0)
            hipLaunchKernelGGL(ppo_gae_runs_apply_kernel<gr_records>, grid, dim3(256), 0, st, rec, H, carry, n_carry);
        else
            hipLaunchKernelGGL(ppo_gae_runs_apply_kernel<gr_composites>, grid, dim3(256), 0, st, gr_composites{lc[l], ld[l]},
                               n[l], carry, n_carry);
    }
    return tw_launched(__func__);
}

int ppo_adv_norm(float *adv, int64_t n, float eps, double *workspace, void *stream) {
    if (!all_set(adv, workspace) || n <= 0) return TW_E_ARG;
    const int nblocks = blocks_capped(n, 1024, 256);         // partial sums: one workgroup per CU at most
    const int nblocks2 = blocks_capped(n, 256, 2048);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(ppo_moments_kernel, dim3(nblocks), dim3(256), 0, st, adv, n, workspace);
    hipLaunchKernelGGL(ppo_normalise_kernel, dim3(nblocks2), dim3(256), 0, st, adv, n, eps, workspace, nblocks);
    return tw_launched(__func__);
}

int ppo_loss_fwd_bwd(const float *probs, const int32_t *action, const float *old_logp, const float *adv,
                     const float *value, const float *target_v, int B, int A, float clip, float ent_coef,
                     float *losses, float *grad_probs, float *grad_value, float *workspace, void *stream) {
    return ppo_loss_fwd_bwd_masked(probs, action, old_logp, adv, value, target_v, B, B, A, clip, ent_coef, losses,
                                   grad_probs, grad_value, workspace, stream);
}

int ppo_loss_fwd_bwd_masked(const float *probs, const int32_t *action, const float *old_logp, const float *adv,
                            const float *value, const float *target_v, int B, int n_valid, int A, float clip,
                            float ent_coef, float *losses, float *grad_probs, float *grad_value, float *workspace,
                            void *stream) {
    if (!all_set(probs, action, old_logp, adv, value, target_v, losses, grad_probs, grad_value, workspace) || B <= 0 ||
        A != 5 || n_valid <= 0 || n_valid > B)              // the reference's policy has five actions: the one width built
        return TW_E_ARG;
    const int nblocks = blocks(B, 256);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL((ppo_loss_kernel<5, false>), dim3(nblocks), dim3(256), 0, st, probs, action, old_logp, adv, value,
                       target_v, B, n_valid, clip, ent_coef, grad_probs, grad_value, workspace, (double *)nullptr);
    hipLaunchKernelGGL(ppo_loss_finalize_kernel, dim3(1), dim3(64), 0, st, workspace, nblocks, n_valid, losses);
    return tw_launched(__func__);
}

int ppo_loss_stats_workspace(int B) { return B > 0 ? blocks(B, 256) * LS_NV : TW_E_ARG; }

int ppo_loss_fwd_bwd_stats(const float *probs, const int32_t *action, const float *old_logp, const float *adv,
                           const float *value, const float *target_v, int B, int n_valid, int A, float clip,
                           float ent_coef, float *losses, float *grad_probs, float *grad_value, float *workspace,
                           double *stats, double *stats_workspace, void *stream) {
    if (!all_set(probs, action, old_logp, adv, value, target_v, losses, grad_probs, grad_value, workspace, stats,
                 stats_workspace) || B <= 0 || A != 5 || n_valid <= 0 || n_valid > B ||       // the masked entry's rules
        !aligned_natural(stats, stats_workspace))
        return TW_E_ARG;
    const int nblocks = blocks(B, 256);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL((ppo_loss_kernel<5, true>), dim3(nblocks), dim3(256), 0, st, probs, action, old_logp, adv, value,
                       target_v, B, n_valid, clip, ent_coef, grad_probs, grad_value, workspace, stats_workspace);
    hipLaunchKernelGGL(ppo_loss_stats_finalize_kernel, dim3(1), dim3(64), 0, st, workspace, stats_workspace, nblocks,
                       n_valid, losses, stats);
    return tw_launched(__func__);
}

int ppo_prior_loss_fwd_bwd(const float *probs, const uint8_t *moves, int B, int n_valid, int A, float coef, float *out,
                           int32_t *counts, float *grad_probs, float *workspace, void *stream) {
    if (!all_set(probs, moves, out, counts, grad_probs, workspace) || B <= 0 || n_valid < 0 || n_valid > B ||
        !ppo_actions_ok(A))
        return TW_E_ARG;
    const int nblocks = blocks(B, 256);
    hipStream_t st = (hipStream_t)stream;
    ppo_with_actions(A, [&](auto a) {
        hipLaunchKernelGGL(ppo_prior_partial_kernel<decltype(a)::value>, dim3(nblocks), dim3(256), 0, st, probs, moves, n_valid,
                           workspace);
        hipLaunchKernelGGL(ppo_prior_grad_kernel<decltype(a)::value>, dim3(nblocks), dim3(256), 0, st, probs, moves, B, n_valid,
                           coef, workspace, nblocks, out, counts, grad_probs);
    });
    return tw_launched(__func__);
}

int ppo_gather_stack(const float *frames, int frame_pitch, const float *pos_frames, int N, const int32_t *k_idx,
                     const int32_t *n_idx, const int32_t *age, const float *init_frame, const float *init_pos, int B,
                     float *out, float *pos_out, void *stream) {
    return gather_stack(__func__, frames, frame_pitch, pos_frames, N, k_idx, n_idx, age, init_frame, init_pos, B, out, pos_out,
                        stream);
}

int ppo_gather_stack_u8(const uint8_t *frames, int frame_pitch, const float *pos_frames, int N, const int32_t *k_idx,
                        const int32_t *n_idx, const int32_t *age, const float *init_frame, const float *init_pos, int B,
                        float *out, float *pos_out, void *stream) {
    return gather_stack(__func__, frames, frame_pitch, pos_frames, N, k_idx, n_idx, age, init_frame, init_pos, B, out, pos_out,
                        stream);
}

int ppo_her_relabel_window(const float *pos, const uint8_t *terminated, const uint8_t *truncated, const int32_t *age0,
                           const float *reward, const int32_t *choices, uint64_t seed, uint32_t env_id0, uint32_t step0,
                           int T, int N, int max_goals, int skip, const int64_t *offsets, int32_t *counts, int32_t *out_t,
                           int32_t *out_n, float *out_goal, float *out_reward, uint8_t *out_done, void *stream) {
    if (!all_set(pos, terminated, truncated, age0, reward) || T <= 0 || N <= 0 || max_goals < 0) return TW_E_ARG;
    if (max_goals > 4) return TW_E_ARG;                                  // 4 pick columns / one Philox call
    if (skip < 0 || skip >= HER_MAX_LEN) return TW_E_ARG;
    if (!offsets && !counts) return TW_E_ARG;
    if (offsets && !all_set(out_t, out_n, out_goal, out_reward, out_done)) return TW_E_ARG;
    hipLaunchKernelGGL(ppo_her_kernel, dim3(N), dim3(64), 0, (hipStream_t)stream, pos, terminated, truncated, age0,
                       reward, choices, (uint32_t)seed, (uint32_t)(seed >> 32), env_id0, step0, T, N, max_goals, skip,
                       offsets, counts, out_t, out_n, out_goal, out_reward, out_done);
    return tw_launched(__func__);
}

int ppo_her_relabel(const float *pos, const uint8_t *terminated, const uint8_t *truncated, const int32_t *age0,
                    const float *reward, const int32_t *choices, uint64_t seed, uint32_t env_id0, uint32_t step0, int T,
                    int N, int max_goals, const int64_t *offsets, int32_t *counts, int32_t *out_t, int32_t *out_n,
                    float *out_goal, float *out_reward, uint8_t *out_done, void *stream) {
    return ppo_her_relabel_window(pos, terminated, truncated, age0, reward, choices, seed, env_id0, step0, T, N, max_goals,
                                  0, offsets, counts, out_t, out_n, out_goal, out_reward, out_done, stream);
}

int ppo_her_select(const float *pos, const uint8_t *terminated, const uint8_t *truncated, const int32_t *age0, int T, int N,
                   int max_goals, int skip, int rule, const uint16_t *key16, const int64_t *table, int width, int height,
                   uint64_t seed, uint32_t env_id0, uint32_t step0, int32_t *choices, int64_t *stats, void *stream) {
    if (!all_set(pos, terminated, truncated, age0, choices) || T < 0 || N <= 0 || !ep_count_ok((int64_t)T * N))
        return TW_E_ARG;
    if (max_goals < 1 || max_goals > 4 || skip < 0 || skip >= HER_MAX_LEN) return TW_E_ARG;
    if (rule != PPO_HER_LATE && rule != PPO_HER_KEY16 && rule != PPO_HER_TABLE) return TW_E_ARG;
    if (rule == PPO_HER_KEY16 && !key16) return TW_E_ARG;
    if (rule == PPO_HER_TABLE && (!table || !visit_grid_ok(width, height))) return TW_E_ARG;
    if ((uintptr_t)pos % 8 || !aligned_natural(choices, key16, table, stats)) return TW_E_ARG;
    if (T == 0) return TW_OK;
    hipLaunchKernelGGL(ppo_her_select_kernel, dim3(N), dim3(64), 0, (hipStream_t)stream, pos, terminated, truncated, age0, T,
                       N, max_goals, skip, rule, key16, table, width, height, (uint32_t)seed, (uint32_t)(seed >> 32),
                       env_id0, step0, choices, reinterpret_cast<unsigned long long *>(stats));
    return tw_launched(__func__);
}

int ppo_age_scan(const uint8_t *terminated, const uint8_t *truncated, const int32_t *age0, int T, int N, int32_t *age,
                 void *stream) {
    if (!all_set(terminated, truncated, age0, age) || T <= 0 || N <= 0) return TW_E_ARG;
    hipLaunchKernelGGL(ppo_age_scan_kernel, dim3(blocks(N, 256)), dim3(256), 0, (hipStream_t)stream, terminated,
                       truncated, age0, T, N, age);
    return tw_launched(__func__);
}

int ppo_episode_scan(const float *reward, const uint8_t *terminated, const uint8_t *truncated, int T, int N,
                     double *carry_return, int32_t *carry_length, double *ep_return, int32_t *ep_length, void *stream) {
    if (!all_set(reward, terminated, truncated, carry_return, carry_length) || T <= 0 || N <= 0 ||
        !ep_count_ok((int64_t)T * N) || !aligned_natural(reward, carry_return, carry_length, ep_return, ep_length))
        return TW_E_ARG;
    hipLaunchKernelGGL(ppo_episode_scan_kernel, dim3(blocks(N, 64)), dim3(64), 0, (hipStream_t)stream, reward, terminated,
                       truncated, T, N, carry_return, carry_length, ep_return, ep_length);
    return tw_launched(__func__);
}

int ppo_episode_summary_workspace(int T, int N) {
    if (T <= 0 || N <= 0 || !ep_count_ok((int64_t)T * N)) return TW_E_ARG;
    return ep_summary_blocks((int64_t)T * N) * EP_NV;
}

int ppo_episode_summary(const double *ep_return, const int32_t *ep_length, const uint8_t *terminated,
                        const uint8_t *truncated, const float *reward, const int32_t *action, int A, int T, int N,
                        double keep, double gain, double *score, double *summary, int64_t *action_hist,
                        int64_t *reward_hist, double *workspace, void *stream) {
    if (!all_set(ep_return, ep_length, terminated, truncated, reward, summary, reward_hist, workspace) || T <= 0 || N <= 0 ||
        !ppo_actions_ok(A) || !ep_count_ok((int64_t)T * N) ||
        !aligned_natural(ep_return, ep_length, reward, action, score, summary, action_hist, reward_hist, workspace))
        return TW_E_ARG;
    const int64_t M = (int64_t)T * N;
    const int nblocks = ep_summary_blocks(M);
    const int64_t per_block = (M + nblocks - 1) / nblocks;
    const int per_thread = blocks(per_block, 256);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(ppo_episode_partial_kernel, dim3(nblocks), dim3(256), 0, st, ep_return, ep_length, terminated,
                       truncated, reward, action, M, per_block, per_thread, keep, gain, workspace);
    hipLaunchKernelGGL(ppo_episode_finalize_kernel, dim3(1), dim3(64), 0, st, workspace, nblocks, A, score, summary,
                       action_hist, reward_hist);
    return tw_launched(__func__);
}

int ppo_bias_relu_nhwc(float *y, const float *bias, int64_t n_pixels, int C, void *stream) {
    if (!all_set(y, bias) || n_pixels <= 0 || C <= 0 || (C & 3) || !aligned16(y, bias)) return TW_E_ARG;
    const size_t n4 = (size_t)n_pixels * (C / 4);
    hipLaunchKernelGGL(ppo_bias_relu_kernel, dim3(blocks_capped((int64_t)n4, 256, 8192)), dim3(256), 0, (hipStream_t)stream,
                       f4(y), f4(bias), n4, C / 4);
    return tw_launched(__func__);
}

int ppo_relu_bwd_bias_grad_nhwc_blocks(int64_t n_pixels, int C) {
    if (n_pixels <= 0 || C <= 0 || (C & 3) || C > 256) return TW_E_ARG;
    return blocks_capped(n_pixels, 512, 4096);                // >= 512 pixels per block
}

int ppo_relu_bwd_bias_grad_nhwc(const float *gy, const float *y, float *gx, float *partial, int64_t n_pixels, int C,
                                void *stream) {
    const int nb = ppo_relu_bwd_bias_grad_nhwc_blocks(n_pixels, C);
    if (nb <= 0 || !all_set(gy, y, gx, partial) || !aligned16(gy, y, gx, partial)) return TW_E_ARG;
    const int ppb = blocks(n_pixels, nb);                     // pixels per block
    hipLaunchKernelGGL(ppo_relu_bwd_bias_grad_kernel, dim3(nb), dim3(256), 0, (hipStream_t)stream, f4(gy), f4(y), f4(gx),
                       f4(partial), (size_t)n_pixels, C / 4, ppb);
    return tw_launched(__func__);
}

int ppo_conv1_up4_bias_relu(const float *frames, int B, int F, const float *folded_w, const float *bias, float *out,
                            void *stream) {
    return ppo_conv1_up4_bias_relu_c(frames, B, F, 64, folded_w, bias, out, stream);
}

int ppo_conv1_up4_bias_relu_c(const float *frames, int B, int F, int C_out, const float *folded_w, const float *bias,
                              float *out, void *stream) {
    if (!all_set(frames, folded_w, bias, out) || B <= 0 || !aligned16(out, folded_w, bias)) return TW_E_ARG;
    auto launch = [&](auto f, auto cq) {
        hipLaunchKernelGGL((ppo_conv1_up4_kernel<decltype(f)::value, decltype(cq)::value>), dim3(B), dim3(256), 0,
                           (hipStream_t)stream, frames, f4(folded_w), f4(bias), f4(out), B);
    };
    if (F == 4 && C_out == 64) launch(int_c<4>{}, int_c<16>{});
    else if (F == 8 && C_out == 64) launch(int_c<8>{}, int_c<16>{});
    else if (F == 1 && C_out == 16) launch(int_c<1>{}, int_c<4>{});
    else return TW_E_ARG;
    return tw_launched(__func__);
}

int ppo_conv1_up4_bwd_groups(int B) { return B <= 0 ? TW_E_ARG : blocks_capped(B, 1, 256); }

int ppo_conv1_up4_bwd(const float *frames, int B, int F, const float *gy, const float *y, float *gw_partial,
                      float *gb_partial, void *stream) {
    const int groups = ppo_conv1_up4_bwd_groups(B);
    if (groups <= 0 || !all_set(frames, gy, y, gw_partial, gb_partial) || !aligned16(gy, y, gw_partial, gb_partial))
        return TW_E_ARG;
    auto launch = [&](auto f) {
        hipLaunchKernelGGL(ppo_conv1_up4_bwd_kernel<decltype(f)::value>, dim3(groups, 4), dim3(256), 0, (hipStream_t)stream,
                           frames, f4(gy), f4(y), f4(gw_partial), f4(gb_partial), B);
    };
    if (F == 4) launch(int_c<4>{});
    else if (F == 8) launch(int_c<8>{});
    else return TW_E_ARG;
    return tw_launched(__func__);
}

int ppo_decoder_frames(const float *z, int n_frames, const float *w1, const float *b1, const float *w2, const float *b2,
                       const float *kfold, float b3, float *frames, void *stream) {
    if (!all_set(z, w1, b1, w2, b2, kfold, frames) || n_frames <= 0) return TW_E_ARG;
    const int grid = blocks_capped(n_frames, 1, 512);          // 120 KB of LDS: one workgroup per CU, two rounds of them
    hipLaunchKernelGGL(ppo_decoder_frames_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, z, n_frames, w1, b1, w2,
                       b2, kfold, b3, frames);
    return tw_launched(__func__);
}

int ppo_lstm_cell(const float *gates_a, const float *gates_b, long long ldb, const float *bias, float *c, float *h, int B,
                  int H, void *stream) {
    if ((!gates_a && !gates_b) || !all_set(c, h) || B <= 0 || H <= 0 || (H & 3) || !aligned16(gates_a, gates_b, bias, c, h))
        return TW_E_ARG;
    if (gates_b && ((ldb & 3) || ldb < 4LL * H)) return TW_E_ARG;
    const long long n = (long long)B * (H / 4);
    if (n > 0x7fffffffLL) return TW_E_ARG;
    hipLaunchKernelGGL(ppo_lstm_cell_kernel, dim3(blocks(n, 256)), dim3(256), 0, (hipStream_t)stream, f4(gates_a),
                       f4(gates_b), ldb / 4, f4(bias), f4(c), f4(h), B, H / 4);
    return tw_launched(__func__);
}

}  // extern "C"
