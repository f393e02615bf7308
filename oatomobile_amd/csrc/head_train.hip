// The density head of K ensemble members trained on cached encoder features (include/rip_head.h).
//
// With the encoder frozen in eval mode its output feat [128] per (member, observation) is a constant, and what is left
// of ImitativeModel's training step (dim/train.py:175-213) is the merger (dim/model.py:56-61: three Linear + ReLU,
// 133 -> 64 -> 64 -> 64, the last ReLU included) and the teacher-forced inverse of the flow (sequence.py:153-216):
// 32 164 parameters per member, the tail of arch.packed_spec().
//
//   head_train_kernel<TRAIN>   one wave per (member k = blockIdx.y, row b), lane j = hidden unit j, grid-stride over the
//                              rows.  Merger weights (and for the adjoint their transposes) and the flow head's W1 are
//                              staged in LDS once per workgroup, W_hh lives in registers (FlowRegs), the flow's tape in
//                              LDS per wave.  Forward: q = log_prob - logabsdet and z.  TRAIN: the adjoint with
//                              cotangent -1/B down to dh1 and per row the vectors whose outer products are the weight
//                              gradients (the flow's as flow_train_kernel records them, plus the merger's three pairs).
//   head_wgrad_kernel          every dW = sum_r a_r (x) b_r and bias column sum of all K members in one launch: a
//                              workgroup owns an 8 x 64 tile of one tensor, its four waves take the rows r = w, w + 4,
//                              ... in order and their four sums are added in wave order.  No atomics: the order is fixed
//                              by (B, shapes) alone, whatever K.
//   head_loss_kernel           loss[k] = -mean_b q[k][b], a fixed tree.
#include "head_train.h"

#include <algorithm>

#include "flow.h"
#include "flow_math.h"
#include "flow_wave.h"
#include "train.h"

namespace rip {

namespace {

constexpr int M0_STRIDE = 140;  // floats per LDS row of merger W0 [64][133]: 35 16-byte slots (odd), conflict-free ds_read_b128
constexpr int MS = W1_STRIDE;   // ... and of every [.][64] matrix: 17 slots
constexpr int L_W0 = 0;
constexpr int L_WM1 = L_W0 + 64 * M0_STRIDE;
constexpr int L_WM2 = L_WM1 + 64 * MS;
constexpr int L_FW1 = L_WM2 + 64 * MS;
constexpr int L_EVAL_END = L_FW1 + 32 * MS;     // forward only: 79 360 B
constexpr int L_WT1 = L_EVAL_END;               // W1^T, W2^T of the merger (dh1, dh2)
constexpr int L_WT2 = L_WT1 + 64 * MS;
constexpr int L_TAPE = L_WT2 + 64 * MS;
constexpr int HEAD_TAPE = T * 7 * 64 + T * 8;   // per wave: [t][7][64] lane tape + [t][8] uniforms (flow_train_kernel's)
constexpr int HEAD_WAVES = 4;
constexpr int L_TRAIN_END = L_TAPE + HEAD_WAVES * HEAD_TAPE;  // 143 360 B: one workgroup per CU
static_assert(L_TRAIN_END * 4 <= 160 * 1024, "LDS budget");

// lane j: acc + sum_i wrow[i] x[i] over one LDS row of 64 weights, x broadcast lane by lane
__device__ __forceinline__ float lds_mv64(const float* wrow, float x, float acc) {
#pragma unroll
  for (int i4 = 0; i4 < 16; ++i4) {
    const float4 w = *reinterpret_cast<const float4*>(wrow + 4 * i4);
    acc = fmaf(w.x, rl(x, 4 * i4 + 0), acc);
    acc = fmaf(w.y, rl(x, 4 * i4 + 1), acc);
    acc = fmaf(w.z, rl(x, 4 * i4 + 2), acc);
    acc = fmaf(w.w, rl(x, 4 * i4 + 3), acc);
  }
  return acc;
}

// FlowRegs of lane j from the reference's tensor layout (a member's head vector)
__device__ __forceinline__ void load_flow_regs_packed(FlowRegs& W, const float* __restrict__ hk, int lane) {
#pragma unroll
  for (int g = 0; g < 3; ++g) {
    const float4* p = reinterpret_cast<const float4*>(hk + H_WHH + (g * 64 + lane) * 64);
#pragma unroll
    for (int i4 = 0; i4 < 16; ++i4) {
      const float4 v = p[i4];
      W.whh[g][4 * i4 + 0] = v.x;
      W.whh[g][4 * i4 + 1] = v.y;
      W.whh[g][4 * i4 + 2] = v.z;
      W.whh[g][4 * i4 + 3] = v.w;
    }
    W.wih[g][0] = hk[H_WIH + (g * 64 + lane) * 2 + 0];
    W.wih[g][1] = hk[H_WIH + (g * 64 + lane) * 2 + 1];
    W.bih[g] = hk[H_BIH + g * 64 + lane];
    W.bhh[g] = hk[H_BHH + g * 64 + lane];
  }
  W.b1 = hk[H_L0B + (lane & 31)];
  W.w2a = hk[H_L2W + (2 * (lane >> 5) + 0) * 32 + (lane & 31)];
  W.w2b = hk[H_L2W + (2 * (lane >> 5) + 1) * 32 + (lane & 31)];
#pragma unroll
  for (int c = 0; c < 4; ++c) W.b2[c] = hk[H_L2B + c];
}

// [rows][64] row-major -> LDS rows of MS floats
__device__ __forceinline__ void stage_rows64(float* dst, const float* __restrict__ src, int rows, int tid, int nthreads) {
  const float4* s4 = reinterpret_cast<const float4*>(src);
  for (int e = tid; e < rows * 16; e += nthreads) {
    const int m = e >> 4, c = e & 15;
    *reinterpret_cast<float4*>(dst + m * MS + 4 * c) = s4[e];
  }
}
// [64][64] row-major -> its transpose in LDS rows of MS floats
__device__ __forceinline__ void stage_transposed64(float* dst, const float* __restrict__ src, int tid, int nthreads) {
  for (int e = tid; e < 64 * 64; e += nthreads) {
    const int j = e >> 6, i = e & 63;
    dst[i * MS + j] = src[e];
  }
}

template <bool TRAIN>
__global__ __launch_bounds__(HEAD_WAVES * 64) void head_train_kernel(HeadArgs a, float cot, float* __restrict__ rec_flow,
                                                                      float* __restrict__ rec_m) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nw = blockDim.x >> 6;
  const int k = blockIdx.y, B = a.B;
  const float* hk = a.head + (size_t)k * HEAD_NUMEL;
  for (int e = tid; e < 64 * HEAD_IN; e += blockDim.x) {
    const int j = e / HEAD_IN, i = e - j * HEAD_IN;
    smem[L_W0 + j * M0_STRIDE + i] = hk[H_M0W + e];
  }
  stage_rows64(smem + L_WM1, hk + H_M1W, 64, tid, blockDim.x);
  stage_rows64(smem + L_WM2, hk + H_M2W, 64, tid, blockDim.x);
  stage_rows64(smem + L_FW1, hk + H_L0W, 32, tid, blockDim.x);
  if (TRAIN) {
    stage_transposed64(smem + L_WT1, hk + H_M1W, tid, blockDim.x);
    stage_transposed64(smem + L_WT2, hk + H_M2W, tid, blockDim.x);
  }
  FlowRegs W;
  load_flow_regs_packed(W, hk, lane);
  const float bm0 = hk[H_M0B + lane], bm1 = hk[H_M1B + lane], bm2 = hk[H_M2B + lane];
  __syncthreads();
  const float* w0row = smem + L_W0 + lane * M0_STRIDE;
  const float* wm1row = smem + L_WM1 + lane * MS;
  const float* wm2row = smem + L_WM2 + lane * MS;
  const float* w1row = smem + L_FW1 + (lane & 31) * MS;
  float* tp = smem + L_TAPE + wave * HEAD_TAPE;  // TRAIN only
  float* tu = tp + T * 7 * 64;
  const bool upper = lane >= 32;
  for (int row = blockIdx.x * nw + wave; row < B; row += gridDim.x * nw) {
    const size_t kb = (size_t)k * B + row;
    const long long r = a.rows != nullptr ? a.rows[kb] : (long long)row;
    if (r < 0 || r >= a.n) {  // a row outside the cache: NaN for this (member, row) and through the records for the member
      const float nan = __int_as_float(0x7fc00000);
      if (lane == 0) a.q_rows[kb] = nan;
      if (a.z != nullptr) a.z[kb * 64 + lane] = nan;
      if (TRAIN) {
        for (int e = lane; e < FLOW_TRAIN_ROW_FLOATS; e += 64) rec_flow[kb * FLOW_TRAIN_ROW_FLOATS + e] = nan;
        for (int e = lane; e < HEAD_MREC; e += 64) rec_m[kb * HEAD_MREC + e] = nan;
      }
      continue;
    }
    // ---------------- merger: merged = cat(feat, vec), three Linear + ReLU ----------------
    const float* fr = a.feat + ((size_t)k * a.n + r) * 128;
    const float m0 = fr[lane], m1 = fr[64 + lane];
    const float m2 = lane < 5 ? a.vec[(size_t)r * 5 + lane] : 0.f;
    float acc = lds_mv64(w0row, m0, bm0);
    acc = lds_mv64(w0row + 64, m1, acc);
    {
      const float4 w = *reinterpret_cast<const float4*>(w0row + 128);
      acc = fmaf(w.x, rl(m2, 0), acc);
      acc = fmaf(w.y, rl(m2, 1), acc);
      acc = fmaf(w.z, rl(m2, 2), acc);
      acc = fmaf(w.w, rl(m2, 3), acc);
      acc = fmaf(w0row[132], rl(m2, 4), acc);
    }
    const float h1 = fmaxf(acc, 0.f);
    const float h2 = fmaxf(lds_mv64(wm1row, h1, bm1), 0.f);
    const float zv = fmaxf(lds_mv64(wm2row, h2, bm2), 0.f);  // activate_final=True (dim/model.py:56-61)
    if (a.z != nullptr) a.z[kb * 64 + lane] = zv;
    // ---------------- target: dense, or every stride-th waypoint of the cached future (+ noise) ----------------
    float yv[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      if (a.y != nullptr) {
        yv[c] = a.y[kb * 8 + c];
      } else {
        yv[c] = a.future[((size_t)r * a.L + (size_t)(c >> 1) * a.stride) * 2 + (c & 1)];
        if (a.noise != nullptr) yv[c] += a.noise[kb * 8 + c];
      }
    }
    // ---------------- flow, teacher-forced inverse (flow_train_kernel's arithmetic) ----------------
    float h = zv;
    float u0 = 0.f, u1 = 0.f, sq = 0.f, lad = 0.f;
#pragma unroll
    for (int t = 0; t < T; ++t) {
      float gh[3], a1 = 0.f;
      matvec<true, false>(W, w1row, h, gh, a1);
      const float gir = fmaf(W.wih[0][1], u1, fmaf(W.wih[0][0], u0, W.bih[0]));
      const float giz = fmaf(W.wih[1][1], u1, fmaf(W.wih[1][0], u0, W.bih[1]));
      const float gin = fmaf(W.wih[2][1], u1, fmaf(W.wih[2][0], u0, W.bih[2]));
      const float rg = sigmoidf_(gir + gh[0]);
      const float zg = sigmoidf_(giz + gh[1]);
      const float n = tanhf_(fmaf(rg, gh[2], gin));
      const float hn = fmaf(zg, h - n, n);
      float* tl = tp + t * 7 * 64 + lane;
      if (TRAIN) {
        tl[0 * 64] = h;
        tl[1 * 64] = rg;
        tl[2 * 64] = zg;
        tl[3 * 64] = n;
        tl[4 * 64] = gh[2];
      }
      h = hn;
      float ghx[3];
      matvec<false, true>(W, w1row, h, ghx, a1);
      if (TRAIN) {
        tl[5 * 64] = a1;
        tl[6 * 64] = h;
      }
      float o0, o1, o2, o3;
      head_finish(W, a1, o0, o1, o2, o3);
      const float s0 = softplusf_(o2) + 1e-3f, s1 = softplusf_(o3) + 1e-3f;  // sequence.py:193
      const float y0 = yv[2 * t], y1 = yv[2 * t + 1];
      const float x0 = (y0 - (u0 + o0)) * rcpf_(s0), x1 = (y1 - (u1 + o1)) * rcpf_(s1);  // :196
      sq = fmaf(x0, x0, fmaf(x1, x1, sq));
      lad += __logf(s0 * s1);
      if (TRAIN && lane == 0) {
        float* q8 = tu + t * 8;
        q8[0] = x0;
        q8[1] = x1;
        q8[2] = s0;
        q8[3] = s1;
        q8[4] = softplus_gradf_(o2);
        q8[5] = softplus_gradf_(o3);
        q8[6] = u0;
        q8[7] = u1;
      }
      u0 = y0;  // teacher forcing, :201
      u1 = y1;
    }
    if (lane == 0) a.q_rows[kb] = (-0.5f * sq - 4.0f * LOG_2PI) - lad;
    if (!TRAIN) continue;
    __builtin_amdgcn_wave_barrier();
    // ---------------- adjoint of the flow with cotangent cot = -1/B ----------------
    float dhdir = 0.f, dpr = 0.f, dpz = 0.f, dghn = 0.f;
#pragma unroll 1
    for (int t = T - 1; t >= 0; --t) {
      const float* q8 = tu + t * 8;
      const float x0 = q8[0], x1 = q8[1], s0 = q8[2], s1 = q8[3], sg0 = q8[4], sg1 = q8[5];
      const float i0 = rcpf_(s0), i1 = rcpf_(s1);
      // q = -0.5 |x|^2 - sum log s:  dq/ddloc = x / s,  dq/ds = (x^2 - 1) / s  (then through softplus)
      const float dd0 = cot * x0 * i0, dd1 = cot * x1 * i1;
      const float dos0 = cot * (x0 * x0 - 1.0f) * i0 * sg0, dos1 = cot * (x1 * x1 - 1.0f) * i1 * sg1;
      const float* tl = tp + t * 7 * 64 + lane;
      const float a1 = tl[5 * 64];
      const float part = W.w2a * (upper ? dos0 : dd0) + W.w2b * (upper ? dos1 : dd1);
      float da1 = xor32_sum(part);
      da1 = a1 > 0.f ? da1 : 0.f;
      const float da1h = upper ? 0.f : da1;  // rows of W1 are duplicated in both halves
      const float dh = transposed_matvec(W, w1row, da1h, dpr, dpz, dghn, lane) + dhdir;
      float dpn;
      gru_adjoint(dh, tl[0 * 64], tl[1 * 64], tl[2 * 64], tl[3 * 64], tl[4 * 64], dhdir, dpr, dpz, dpn, dghn);
      float* rc = rec_flow + (kb * T + t) * FLOW_TRAIN_REC;
      rc[0 * 64 + lane] = dpr;   // dgi = (d pre_r, d pre_z, d pre_n)
      rc[1 * 64 + lane] = dpz;
      rc[2 * 64 + lane] = dpn;
      rc[192 + 0 * 64 + lane] = dpr;  // dgh = (d pre_r, d pre_z, d gh_n)
      rc[192 + 1 * 64 + lane] = dpz;
      rc[192 + 2 * 64 + lane] = dghn;
      rc[384 + lane] = tl[0 * 64];
      if (lane < 2) rc[448 + lane] = q8[6 + lane];
      if (lane < 32) {
        rc[450 + lane] = da1;
        rc[550 + lane] = fmaxf(a1, 0.f);
      }
      rc[482 + lane] = tl[6 * 64];
      if (lane < 4) rc[546 + lane] = lane == 0 ? dd0 : (lane == 1 ? dd1 : (lane == 2 ? dos0 : dos1));
    }
    const float dz = transposed_matvec(W, w1row, 0.f, dpr, dpz, dghn, lane) + dhdir;
    // ---------------- adjoint of the merger down to dh1 (the features are constants) ----------------
    const float dzm = zv > 0.f ? dz : 0.f;
    const float dh2 = lds_mv64(smem + L_WT2 + lane * MS, dzm, 0.f);
    const float dh2m = h2 > 0.f ? dh2 : 0.f;
    const float dh1 = lds_mv64(smem + L_WT1 + lane * MS, dh2m, 0.f);
    const float dh1m = h1 > 0.f ? dh1 : 0.f;
    float* rm = rec_m + kb * HEAD_MREC;
    rm[HM_DZ + lane] = dzm;
    rm[HM_H2 + lane] = h2;
    rm[HM_DH2 + lane] = dh2m;
    rm[HM_H1 + lane] = h1;
    rm[HM_DH1 + lane] = dh1m;
    rm[HM_IN + lane] = m0;
    rm[HM_IN + 64 + lane] = m1;
    if (lane < 5) rm[HM_IN + 128 + lane] = m2;
    __builtin_amdgcn_wave_barrier();
  }
}

// ------------------------------------------------------------------------------------------
// weight gradients from the records
// ------------------------------------------------------------------------------------------
// One tensor of the head as a sum of outer products: out[i * si + j * sj] = sum_r a_r[i] * b_r[j], 0 <= i < I, 0 <= j < J,
// a_r = record r at float a_off (a_off < 0: ones -> a column sum), b_r likewise; flow: the records are the flow's (4B rows
// of FLOW_TRAIN_REC floats), else the merger's (B rows of HEAD_MREC).  tile0: the tensor's first 8 x 64 tile in the grid.
struct WgradSeg {
  int out, I, J, si, sj, a_off, b_off, flow, tile0;
};
constexpr int WGRAD_SEGS = 14;
constexpr int WGRAD_TI = 8, WGRAD_TJ = 64, WGRAD_WAVES = 4;
struct WgradSegs {
  WgradSeg s[WGRAD_SEGS];
  int tiles;
};

WgradSegs wgrad_segments() {
  WgradSegs g;
  const WgradSeg table[WGRAD_SEGS] = {
      {H_M0W, 64, HEAD_IN, HEAD_IN, 1, HM_DH1, HM_IN, 0, 0},  // dW0 = dh1m (x) merged
      {H_M0B, 1, 64, 0, 1, -1, HM_DH1, 0, 0},
      {H_M1W, 64, 64, 64, 1, HM_DH2, HM_H1, 0, 0},            // dW1 = dh2m (x) h1
      {H_M1B, 1, 64, 0, 1, -1, HM_DH2, 0, 0},
      {H_M2W, 64, 64, 64, 1, HM_DZ, HM_H2, 0, 0},             // dW2 = dzm (x) h2
      {H_M2B, 1, 64, 0, 1, -1, HM_DZ, 0, 0},
      {H_WIH, 2, 192, 1, 2, 448, 0, 1, 0},                    // dW_ih[j][i] = dgi_j u_i (transposed: 192 lanes wide)
      {H_WHH, 192, 64, 64, 1, 192, 384, 1, 0},                // dW_hh = dgh (x) hprev
      {H_BIH, 1, 192, 0, 1, -1, 0, 1, 0},
      {H_BHH, 1, 192, 0, 1, -1, 192, 1, 0},
      {H_L0W, 32, 64, 64, 1, 450, 482, 1, 0},                 // dW1 = da1 (x) h
      {H_L0B, 1, 32, 0, 1, -1, 450, 1, 0},
      {H_L2W, 4, 32, 32, 1, 546, 550, 1, 0},                  // dW2 = do (x) relu(a1)
      {H_L2B, 1, 4, 0, 1, -1, 546, 1, 0},
  };
  int tiles = 0;
  for (int i = 0; i < WGRAD_SEGS; ++i) {
    g.s[i] = table[i];
    g.s[i].tile0 = tiles;
    tiles += ((table[i].I + WGRAD_TI - 1) / WGRAD_TI) * ((table[i].J + WGRAD_TJ - 1) / WGRAD_TJ);
  }
  g.tiles = tiles;
  return g;
}

__global__ __launch_bounds__(WGRAD_WAVES * 64) void head_wgrad_kernel(WgradSegs segs, const float* __restrict__ rec_flow,
                                                                       const float* __restrict__ rec_m, int B,
                                                                       float* __restrict__ grads) {
  __shared__ float part[WGRAD_WAVES][WGRAD_TI][WGRAD_TJ];
  const int k = blockIdx.y, tile = blockIdx.x;
  int si = 0;
  for (int i = 1; i < WGRAD_SEGS; ++i)
    if (tile >= segs.s[i].tile0) si = i;
  const WgradSeg S = segs.s[si];
  const int tj = (S.J + WGRAD_TJ - 1) / WGRAD_TJ, lt = tile - S.tile0;
  const int i0 = (lt / tj) * WGRAD_TI, j0 = (lt % tj) * WGRAD_TJ;
  const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int R = S.flow ? T * B : B, stride = S.flow ? FLOW_TRAIN_REC : HEAD_MREC;
  const float* base = S.flow ? rec_flow + (size_t)k * B * FLOW_TRAIN_ROW_FLOATS : rec_m + (size_t)k * B * HEAD_MREC;
  const int j = min(j0 + lane, S.J - 1);  // lanes and rows past the tensor's edge read its last element and store nothing
  int ia[WGRAD_TI];
#pragma unroll
  for (int ii = 0; ii < WGRAD_TI; ++ii) ia[ii] = min(i0 + ii, S.I - 1);
  float acc[WGRAD_TI];
#pragma unroll
  for (int ii = 0; ii < WGRAD_TI; ++ii) acc[ii] = 0.f;
#pragma unroll 4
  for (int r = w; r < R; r += WGRAD_WAVES) {
    const float* rp = base + (size_t)r * stride;
    const float bv = S.b_off >= 0 ? rp[S.b_off + j] : 1.0f;
#pragma unroll
    for (int ii = 0; ii < WGRAD_TI; ++ii) acc[ii] = fmaf(S.a_off >= 0 ? rp[S.a_off + ia[ii]] : 1.0f, bv, acc[ii]);
  }
#pragma unroll
  for (int ii = 0; ii < WGRAD_TI; ++ii) part[w][ii][lane] = acc[ii];
  __syncthreads();
  for (int e = threadIdx.x; e < WGRAD_TI * WGRAD_TJ; e += blockDim.x) {
    const int ii = e >> 6, l = e & 63;
    const float sum = ((part[0][ii][l] + part[1][ii][l]) + part[2][ii][l]) + part[3][ii][l];
    if (i0 + ii < S.I && j0 + l < S.J) grads[(size_t)k * HEAD_NUMEL + S.out + (i0 + ii) * S.si + (j0 + l) * S.sj] = sum;
  }
}

__global__ __launch_bounds__(256) void head_loss_kernel(const float* __restrict__ q_rows, int B, float* __restrict__ loss) {
  __shared__ float p[256];
  const int k = blockIdx.x, tid = threadIdx.x;
  float s = 0.f;
  for (int b = tid; b < B; b += 256) s += q_rows[(size_t)k * B + b];
  p[tid] = s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) p[tid] += p[tid + o];
    __syncthreads();
  }
  if (tid == 0) loss[k] = -p[0] / (float)B;
}

}  // namespace

size_t head_workspace_bytes(int K, int max_batch) {
  return (size_t)K * max_batch * (FLOW_TRAIN_ROW_FLOATS + HEAD_MREC) * sizeof(float);
}

hipError_t launch_head_step(const HeadArgs& a, float* grads, void* workspace, hipStream_t s) {
  const bool train = grads != nullptr;
  float* rec_flow = static_cast<float*>(workspace);
  float* rec_m = train ? rec_flow + (size_t)a.K * a.B * FLOW_TRAIN_ROW_FLOATS : nullptr;
  const int gx = std::max(1, std::min((a.B + HEAD_WAVES - 1) / HEAD_WAVES, device_cu_count() / a.K));
  const dim3 grid(gx, a.K), block(HEAD_WAVES * 64);
  const float cot = -1.0f / (float)a.B;
  if (train) {
    hipError_t e = allow_lds(reinterpret_cast<const void*>(head_train_kernel<true>));
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(head_train_kernel<true>, grid, block, L_TRAIN_END * sizeof(float), s, a, cot, rec_flow, rec_m);
    static const WgradSegs segs = wgrad_segments();
    hipLaunchKernelGGL(head_wgrad_kernel, dim3(segs.tiles, a.K), dim3(WGRAD_WAVES * 64), 0, s, segs, rec_flow, rec_m, a.B,
                       grads);
  } else {
    hipError_t e = allow_lds(reinterpret_cast<const void*>(head_train_kernel<false>));
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(head_train_kernel<false>, grid, block, L_EVAL_END * sizeof(float), s, a, cot, rec_flow, rec_m);
  }
  hipLaunchKernelGGL(head_loss_kernel, dim3(a.K), dim3(256), 0, s, a.q_rows, a.B, a.loss);
  return hipGetLastError();
}

}  // namespace rip
