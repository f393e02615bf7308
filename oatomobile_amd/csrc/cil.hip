// Decoder of the conditional-imitation-learning model for gfx950.
//
// Reference: BehaviouralModel.forward (oatomobile/baselines/torch/cil/model.py:68-127) after the encoder:
//   z = merger(cat(features[128], velocity[3], is_at_traffic_light, traffic_light_state, mode))   (:88-101; MLP
//       134 -> 64 -> 64 -> 64, ReLU after every layer, :50-56)
//   x = 0; for t in range(T): z = GRUCell(x, z); x = x + Linear(z); y[t] = x                       (:106-125)
// One wavefront per sample, lane j = hidden unit j (the wave-per-chain layout of flow.hip): W_hh rows live in
// registers (192 per lane), the hidden state is broadcast through LDS, the 2-wide head is a wave reduction.  The
// whole decode is ~0.5 MFLOP per sample; it is launch latency, not throughput, that matters here, so everything after
// the encoder is this ONE kernel.
//
// Training (cil/train.py:168-190): cil_train_kernel below is this decoder's forward with a tape, the L1 loss
// cotangent and the backward-through-time; the encoder / merger halves of the step are the DIM trainer's (train.hip).
//
// Weight blob (fp32, arch.py:cil_decoder_spec order): W0[64][134] b0[64] W1[64][64] b1[64] W2[64][64] b2[64]
// W_ih[192][2] W_hh[192][64] b_ih[192] b_hh[192] W_out[2][64] b_out[2].  torch.nn.GRUCell gate order (r, z, n).
#include <hip/hip_runtime.h>

#include "flow.h"
#include "flow_math.h"
#include "train.h"

namespace rip {

namespace {

constexpr int NF = 128, NV = 6, NIN = NF + NV, H = 64;
constexpr int OFF_W0 = 0, OFF_B0 = OFF_W0 + H * NIN, OFF_W1 = OFF_B0 + H, OFF_B1 = OFF_W1 + H * H;
constexpr int OFF_W2 = OFF_B1 + H, OFF_B2 = OFF_W2 + H * H, OFF_WIH = OFF_B2 + H, OFF_WHH = OFF_WIH + 3 * H * 2;
constexpr int OFF_BIH = OFF_WHH + 3 * H * H, OFF_BHH = OFF_BIH + 3 * H, OFF_WO = OFF_BHH + 3 * H, OFF_BO = OFF_WO + 2 * H;
constexpr int CIL_BLOB = OFF_BO + 2;  // 30146 floats
constexpr int WAVES = 4;

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}

__global__ __launch_bounds__(WAVES * 64) void cil_decode_kernel(const float* __restrict__ feat,
                                                                const float* __restrict__ vec,
                                                                const float* __restrict__ w, int B, int T,
                                                                float* __restrict__ y) {
  __shared__ float act[WAVES][NIN + 2];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int b = blockIdx.x * WAVES + wave;
  if (b >= B) return;
  float* a = act[wave];
  // ---- merger input: cat(features, vector inputs)  (cil/model.py:88-98)
  a[lane] = feat[(size_t)b * NF + lane];
  a[64 + lane] = feat[(size_t)b * NF + 64 + lane];
  if (lane < NV) a[NF + lane] = vec[(size_t)b * NV + lane];
  __builtin_amdgcn_wave_barrier();
  // ---- merger: three Linear + ReLU layers, lane j = output unit j
  float h;
  {
    const float* r0 = w + OFF_W0 + lane * NIN;
    float s = w[OFF_B0 + lane];
    for (int i = 0; i < NIN; ++i) s = fmaf(r0[i], a[i], s);
    h = fmaxf(s, 0.f);
  }
  __builtin_amdgcn_wave_barrier();
  a[lane] = h;
  __builtin_amdgcn_wave_barrier();
  {
    const float* r1 = w + OFF_W1 + lane * H;
    float s = w[OFF_B1 + lane];
    for (int i = 0; i < H; ++i) s = fmaf(r1[i], a[i], s);
    h = fmaxf(s, 0.f);
  }
  __builtin_amdgcn_wave_barrier();
  a[lane] = h;
  __builtin_amdgcn_wave_barrier();
  {
    const float* r2 = w + OFF_W2 + lane * H;
    float s = w[OFF_B2 + lane];
    for (int i = 0; i < H; ++i) s = fmaf(r2[i], a[i], s);
    h = fmaxf(s, 0.f);
  }
  // ---- GRU rollout (cil/model.py:106-125); per-lane rows of W_hh / W_ih of gates r, z, n
  float whr[H], whz[H], whn[H];
#pragma unroll
  for (int i = 0; i < H; ++i) {
    whr[i] = w[OFF_WHH + (0 * H + lane) * H + i];
    whz[i] = w[OFF_WHH + (1 * H + lane) * H + i];
    whn[i] = w[OFF_WHH + (2 * H + lane) * H + i];
  }
  const float wir0 = w[OFF_WIH + (0 * H + lane) * 2], wir1 = w[OFF_WIH + (0 * H + lane) * 2 + 1];
  const float wiz0 = w[OFF_WIH + (1 * H + lane) * 2], wiz1 = w[OFF_WIH + (1 * H + lane) * 2 + 1];
  const float win0 = w[OFF_WIH + (2 * H + lane) * 2], win1 = w[OFF_WIH + (2 * H + lane) * 2 + 1];
  const float bir = w[OFF_BIH + lane], biz = w[OFF_BIH + H + lane], bin = w[OFF_BIH + 2 * H + lane];
  const float bhr = w[OFF_BHH + lane], bhz = w[OFF_BHH + H + lane], bhn = w[OFF_BHH + 2 * H + lane];
  const float wo0 = w[OFF_WO + lane], wo1 = w[OFF_WO + H + lane];
  const float bo0 = w[OFF_BO], bo1 = w[OFF_BO + 1];
  float x0 = 0.f, x1 = 0.f;
  for (int t = 0; t < T; ++t) {
    __builtin_amdgcn_wave_barrier();
    a[lane] = h;
    __builtin_amdgcn_wave_barrier();
    float gr = bhr, gz = bhz, gn = bhn;
#pragma unroll
    for (int i = 0; i < H; ++i) {
      const float hi = a[i];
      gr = fmaf(whr[i], hi, gr);
      gz = fmaf(whz[i], hi, gz);
      gn = fmaf(whn[i], hi, gn);
    }
    const float ir = fmaf(wir1, x1, fmaf(wir0, x0, bir));
    const float iz = fmaf(wiz1, x1, fmaf(wiz0, x0, biz));
    const float in = fmaf(win1, x1, fmaf(win0, x0, bin));
    const float r = sigmoidf_(ir + gr);
    const float z = sigmoidf_(iz + gz);
    const float n = tanhf_(fmaf(r, gn, in));
    h = fmaf(z, h - n, n);  // (1 - z) * n + z * h
    // dx = Linear(h) (cil/model.py:118), x = dx + x (:119)
    const float d0 = wave_sum(wo0 * h) + bo0;
    const float d1 = wave_sum(wo1 * h) + bo1;
    x0 += d0;
    x1 += d1;
    if (lane == 0) {
      y[((size_t)b * T + t) * 2] = x0;
      y[((size_t)b * T + t) * 2 + 1] = x1;
    }
  }
}

// ------------------------------------------------------------------------------------------
// Training: the decoder of BehaviouralModel (cil/model.py:104-125) with L1 loss (cil/train.py:176-180) forward and
// backward-through-time, one wavefront per batch row, lane j = hidden unit j (cil_decode_kernel's layout).
//   forward   cil_decode_kernel's arithmetic, operation for operation (W_hh rows read from LDS instead of registers:
//             the same values in the same fma order), taping per step into the row's records (r, z, n, W_hn h + b_hn,
//             dpred lane-locally in the dgi / dgh slots, h_prev, h, x_in in their own), so T is unbounded;
//   loss      l1_rows[b] = sum_t sum_d |pred - target|,  dpred = sign(pred - target) / B (sign(0) = 0: torch's L1
//             backward);
//   backward  reverse t: g_x(t) = dpred_t + g_x(t+1) + W_ih^T dgi(t+1) (the residual x_t = x_{t-1} + out(h_t), and x_t
//             is the input of step t+1), g_h(t) = W_out^T g_x(t) + z(t+1) g_h(t+1) + W_hh^T dgh(t+1), then the GRUCell
//             adjoint (gate order r, z, n; the n gate's hidden-side pre-activation gradient is r * dn_pre);
//             dz = g_h(-1), the adjoint of the initial hidden state (the merger output).
// Records per (row, t) (CIL_TRAIN_REC floats, train.h): dgi 192 | dgh 192 | h_prev 64 | h 64 | x_in 2 | dout 2; the
// trainer forms dW_ih = dgi^T x_in, dW_hh = dgh^T h_prev, dW_out = dout^T h as GEMMs over the B*T records and the
// biases as their column sums.  W_hh^T: lane i needs column i, so W_hh is staged in LDS with rows padded to 65 floats
// (both the row-per-lane forward read and the column-per-lane backward read are bank-conflict free); no weight lives
// in registers across the kernel.
// ------------------------------------------------------------------------------------------
constexpr int TW = 4;           // waves (rows) per workgroup
constexpr int WHH_LD = H + 1;   // LDS row pitch of W_hh
constexpr int REC_DGI = 0, REC_DGH = 3 * H, REC_HPREV = 6 * H, REC_H = 7 * H, REC_XIN = 8 * H, REC_DOUT = 8 * H + 2;
static_assert(REC_DOUT + 2 == CIL_TRAIN_REC, "record layout");

__device__ __forceinline__ float signf_(float e) { return e > 0.f ? 1.f : (e < 0.f ? -1.f : 0.f); }

__global__ __launch_bounds__(TW * 64) void cil_train_kernel(
    const float* __restrict__ wih, const float* __restrict__ whh, const float* __restrict__ bih,
    const float* __restrict__ bhh, const float* __restrict__ wout, const float* __restrict__ bout,
    const float* __restrict__ zin, const float* __restrict__ target, int B, int T, float inv_b, int backward,
    float* __restrict__ pred, float* __restrict__ l1_rows, float* __restrict__ dz, float* __restrict__ rec) {
  __shared__ float ws[3 * H * WHH_LD];
  __shared__ float bc[TW][3 * H];  // per wave: h (forward) / (dr, dz, dghn) (backward) broadcast
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int e = tid; e < 3 * H * H; e += TW * 64) ws[(e >> 6) * WHH_LD + (e & 63)] = whh[e];
  __syncthreads();
  const int b = blockIdx.x * TW + wave;
  if (b >= B) return;
  float* a = bc[wave];
  const float* wr = ws + (0 * H + lane) * WHH_LD;
  const float* wz = ws + (1 * H + lane) * WHH_LD;
  const float* wn = ws + (2 * H + lane) * WHH_LD;
  const float wir0 = wih[(0 * H + lane) * 2], wir1 = wih[(0 * H + lane) * 2 + 1];
  const float wiz0 = wih[(1 * H + lane) * 2], wiz1 = wih[(1 * H + lane) * 2 + 1];
  const float win0 = wih[(2 * H + lane) * 2], win1 = wih[(2 * H + lane) * 2 + 1];
  const float bir = bih[lane], biz = bih[H + lane], bin = bih[2 * H + lane];
  const float bhr = bhh[lane], bhz = bhh[H + lane], bhn = bhh[2 * H + lane];
  const float wo0 = wout[lane], wo1 = wout[H + lane];
  const float bo0 = bout[0], bo1 = bout[1];
  float h = zin[(size_t)b * H + lane];
  float x0 = 0.f, x1 = 0.f, l1 = 0.f;
  // ---------------- forward (cil_decode_kernel's GRU roll-out) + tape ----------------
#pragma unroll 1
  for (int t = 0; t < T; ++t) {
    float* rc = rec + ((size_t)b * T + t) * CIL_TRAIN_REC;
    __builtin_amdgcn_wave_barrier();
    a[lane] = h;
    __builtin_amdgcn_wave_barrier();
    float gr = bhr, gz = bhz, gn = bhn;
#pragma unroll 16
    for (int i = 0; i < H; ++i) {
      const float hi = a[i];
      gr = fmaf(wr[i], hi, gr);
      gz = fmaf(wz[i], hi, gz);
      gn = fmaf(wn[i], hi, gn);
    }
    const float ir = fmaf(wir1, x1, fmaf(wir0, x0, bir));
    const float iz = fmaf(wiz1, x1, fmaf(wiz0, x0, biz));
    const float in = fmaf(win1, x1, fmaf(win0, x0, bin));
    const float r = sigmoidf_(ir + gr);
    const float z = sigmoidf_(iz + gz);
    const float n = tanhf_(fmaf(r, gn, in));
    rc[REC_DGI + 0 * H + lane] = r;  // tape (lane-local; the backward overwrites these slots with dgi / dgh)
    rc[REC_DGI + 1 * H + lane] = z;
    rc[REC_DGI + 2 * H + lane] = n;
    rc[REC_DGH + 0 * H + lane] = gn;
    rc[REC_HPREV + lane] = h;
    if (lane < 2) rc[REC_XIN + lane] = lane == 0 ? x0 : x1;
    h = fmaf(z, h - n, n);  // (1 - z) * n + z * h
    rc[REC_H + lane] = h;
    const float d0 = wave_sum(wo0 * h) + bo0;
    const float d1 = wave_sum(wo1 * h) + bo1;
    x0 += d0;
    x1 += d1;
    const float* tg = target + ((size_t)b * T + t) * 2;
    const float e0 = x0 - tg[0], e1 = x1 - tg[1];
    l1 += fabsf(e0) + fabsf(e1);
    rc[REC_DGH + 1 * H + lane] = signf_(e0) * inv_b;
    rc[REC_DGH + 2 * H + lane] = signf_(e1) * inv_b;
    if (lane == 0 && pred != nullptr) {
      pred[((size_t)b * T + t) * 2] = x0;
      pred[((size_t)b * T + t) * 2 + 1] = x1;
    }
  }
  if (lane == 0) l1_rows[b] = l1;
  if (!backward) return;
  // ---------------- backward through time ----------------
  float gx0 = 0.f, gx1 = 0.f;  // adjoint of x_t, accumulated from the later steps (wave-uniform)
  float gh = 0.f;              // adjoint of h_t through step t+1 (lane j)
#pragma unroll 1
  for (int t = T - 1; t >= 0; --t) {
    float* rc = rec + ((size_t)b * T + t) * CIL_TRAIN_REC;
    const float r = rc[REC_DGI + 0 * H + lane], z = rc[REC_DGI + 1 * H + lane], n = rc[REC_DGI + 2 * H + lane];
    const float ghn = rc[REC_DGH + 0 * H + lane], dp0 = rc[REC_DGH + 1 * H + lane], dp1 = rc[REC_DGH + 2 * H + lane];
    const float hprev = rc[REC_HPREV + lane];
    gx0 += dp0;
    gx1 += dp1;
    const float dh = fmaf(wo1, gx1, fmaf(wo0, gx0, gh));  // W_out^T g_x + recurrent adjoint
    const float dn = dh * (1.0f - z);
    const float dzg = dh * (hprev - n);
    const float dpn = dn * (1.0f - n * n);
    const float dghn = dpn * r;
    const float dpr = dpn * ghn * r * (1.0f - r);
    const float dpz = dzg * z * (1.0f - z);
    rc[REC_DGI + 0 * H + lane] = dpr;
    rc[REC_DGI + 1 * H + lane] = dpz;
    rc[REC_DGI + 2 * H + lane] = dpn;
    rc[REC_DGH + 0 * H + lane] = dpr;
    rc[REC_DGH + 1 * H + lane] = dpz;
    rc[REC_DGH + 2 * H + lane] = dghn;
    if (lane < 2) rc[REC_DOUT + lane] = lane == 0 ? gx0 : gx1;
    // into x_{t-1}, the input of this step: W_ih^T dgi (the residual part of g_x carries over unchanged)
    gx0 += wave_sum(fmaf(win0, dpn, fmaf(wiz0, dpz, wir0 * dpr)));
    gx1 += wave_sum(fmaf(win1, dpn, fmaf(wiz1, dpz, wir1 * dpr)));
    // into h_{t-1}: z * dh + W_hh^T (dr, dz, dghn); lane i reads column i of W_hh
    __builtin_amdgcn_wave_barrier();
    a[lane] = dpr;
    a[H + lane] = dpz;
    a[2 * H + lane] = dghn;
    __builtin_amdgcn_wave_barrier();
    float s = dh * z;
#pragma unroll 16
    for (int j = 0; j < H; ++j) {
      s = fmaf(ws[(0 * H + j) * WHH_LD + lane], a[j], s);
      s = fmaf(ws[(1 * H + j) * WHH_LD + lane], a[H + j], s);
      s = fmaf(ws[(2 * H + j) * WHH_LD + lane], a[2 * H + j], s);
    }
    gh = s;
  }
  dz[(size_t)b * H + lane] = gh;
}

}  // namespace

int cil_blob_floats() { return CIL_BLOB; }

hipError_t launch_cil_decode(const float* feat, const float* vec, const float* w, int B, int T, float* y, hipStream_t s) {
  if (B <= 0 || T <= 0) return hipSuccess;
  hipLaunchKernelGGL(cil_decode_kernel, dim3((B + WAVES - 1) / WAVES), dim3(WAVES * 64), 0, s, feat, vec, w, B, T, y);
  return hipGetLastError();
}

hipError_t launch_cil_train(const float* wih, const float* whh, const float* bih, const float* bhh, const float* wout,
                            const float* bout, const float* z, const float* target, int B, int T, int backward,
                            float* pred, float* l1_rows, float* dz, float* records, hipStream_t s) {
  if (B <= 0 || T <= 0) return hipSuccess;
  hipLaunchKernelGGL(cil_train_kernel, dim3((B + TW - 1) / TW), dim3(TW * 64), 0, s, wih, whh, bih, bhh, wout, bout, z,
                     target, B, T, 1.0f / (float)B, backward, pred, l1_rows, dz, records);
  return hipGetLastError();
}

}  // namespace rip
