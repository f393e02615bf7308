// Device helpers of the wave-per-chain flow kernels (flow.hip, head_train.hip): ONE 64-lane wavefront per chain, lane j
// owns hidden unit j.  The cross-lane reductions, the register-resident GRU weights of one model, the row-resident
// mat-vec and its transposed (reduce-scatter) counterpart, the head's second layer and the GRUCell adjoint.  Everything
// is __forceinline__: a kernel that includes this compiles to the instructions it had when the helpers stood in its
// own file.
#pragma once
#include <hip/hip_runtime.h>

#include "flow.h"

namespace rip {

namespace {

constexpr int T = 4;
constexpr int W1_STRIDE = 68;                 // floats (272 B rows): conflict-free ds_read_b128 across rows
constexpr int W1_LDS = 32 * W1_STRIDE;        // floats per model
constexpr int TAPE_Q = 6;                     // hprev, r, zg, n, ghn, a1
constexpr int TAPE_LANE = T * TAPE_Q * 64;
constexpr int TAPE_UNI = T * 8;               // x0,x1,s0,s1,sg0,sg1,pad,pad
constexpr int TAPE = TAPE_LANE + TAPE_UNI;    // floats per slot

// ------------------------------------------------------------------------------------------
// cross-lane helpers
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ float rl(float v, int lane) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane));
}
template <int CTRL>
__device__ __forceinline__ float dpp(float x) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), CTRL, 0xf, 0xf, true));
}
// sum over each row of 16 lanes, result replicated in the row
__device__ __forceinline__ float row_sum16(float x) {
  x += dpp<0xB1>(x);   // quad_perm [1,0,3,2]
  x += dpp<0x4E>(x);   // quad_perm [2,3,0,1]
  x += dpp<0x141>(x);  // row_half_mirror
  x += dpp<0x140>(x);  // row_mirror
  return x;
}
__device__ __forceinline__ float wave_sum(float x) {
  x = row_sum16(x);
  return (rl(x, 0) + rl(x, 16)) + (rl(x, 32) + rl(x, 48));
}
// x[lane] + x[lane ^ 32]
__device__ __forceinline__ float xor32_sum(float x) {
  auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(x), false, false);
  return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}
// reduce-scatter stages: `lo`/`hi` are this lane's partial sums for two target indices whose lane ids
// differ in bit D; afterwards the lane holds the pair-sum for the index matching its own bit D.
__device__ __forceinline__ float rs32(float lo, float hi) {
  auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(lo), __float_as_uint(hi), false, false);
  return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}
__device__ __forceinline__ float rs16(float lo, float hi) {
  auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(lo), __float_as_uint(hi), false, false);
  return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}
template <int D>
__device__ __forceinline__ float xor_lane(float v) {  // v[lane ^ D] for D in {1,2,4,8}, all DPP (no LDS)
  if (D == 1) return dpp<0xB1>(v);   // quad_perm [1,0,3,2]
  if (D == 2) return dpp<0x4E>(v);   // quad_perm [2,3,0,1]
  if (D == 8) return dpp<0x128>(v);  // row_ror:8
  // D == 4: lanes with bit2 clear read lane+4 (row_shl:4, banks 0/2), the others lane-4 (row_shr:4, banks 1/3)
  int r = __builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x104, 0xf, 0x5, false);
  r = __builtin_amdgcn_update_dpp(r, __float_as_int(v), 0x114, 0xf, 0xA, false);
  return __int_as_float(r);
}
template <int D>
__device__ __forceinline__ float rs_small(float lo, float hi, int lane) {
  const bool up = (lane & D) != 0;
  const float send = up ? lo : hi;
  const float keep = up ? hi : lo;
  return keep + xor_lane<D>(send);
}

// ------------------------------------------------------------------------------------------
// register-resident weights of one model, as seen by lane j
// ------------------------------------------------------------------------------------------
struct FlowRegs {
  float whh[3][64];  // W_hh[g*64+j][0..63]
  float wih[3][2];   // W_ih[g*64+j][d]
  float bih[3], bhh[3];
  float b1;          // b1[j&31]
  float w2a, w2b;    // W2[2*half+{0,1}][j&31]
  float b2[4];
};

__device__ __forceinline__ void load_flow_regs(FlowRegs& W, const float* __restrict__ blob, int lane) {
  const float4* p = reinterpret_cast<const float4*>(blob + FW_WHH);
#pragma unroll
  for (int g = 0; g < 3; ++g) {
#pragma unroll
    for (int i4 = 0; i4 < 16; ++i4) {
      const float4 v = p[(g * 16 + i4) * 64 + lane];
      W.whh[g][4 * i4 + 0] = v.x;
      W.whh[g][4 * i4 + 1] = v.y;
      W.whh[g][4 * i4 + 2] = v.z;
      W.whh[g][4 * i4 + 3] = v.w;
    }
  }
#pragma unroll
  for (int g = 0; g < 3; ++g) {
    W.wih[g][0] = blob[FW_WIH + (g * 2 + 0) * 64 + lane];
    W.wih[g][1] = blob[FW_WIH + (g * 2 + 1) * 64 + lane];
    W.bih[g] = blob[FW_BIH + g * 64 + lane];
    W.bhh[g] = blob[FW_BHH + g * 64 + lane];
  }
  W.b1 = blob[FW_B1 + lane];
  W.w2a = blob[FW_W2 + lane];
  W.w2b = blob[FW_W2 + 64 + lane];
#pragma unroll
  for (int c = 0; c < 4; ++c) W.b2[c] = blob[FW_B2 + c];
}

// stage W1 [32][64] of one model into LDS rows of W1_STRIDE floats (all `nthreads` threads cooperate)
__device__ __forceinline__ void stage_w1(float* lds_w1, const float* __restrict__ blob, int tid, int nthreads) {
  const float4* src = reinterpret_cast<const float4*>(blob + FW_W1);
  for (int e = tid; e < 32 * 16; e += nthreads) {
    const int m = e >> 4, c = e & 15;
    *reinterpret_cast<float4*>(lds_w1 + m * W1_STRIDE + 4 * c) = src[e];
  }
}

// gh[g] = b_hh[g] + W_hh[g] h   and/or   a1 = b1 + W1[m] h    (one broadcast sweep over h)
template <bool WITH_GH, bool WITH_A1>
__device__ __forceinline__ void matvec(const FlowRegs& W, const float* w1row, float h, float (&gh)[3], float& a1) {
  if (WITH_GH) {
    gh[0] = W.bhh[0];
    gh[1] = W.bhh[1];
    gh[2] = W.bhh[2];
  }
  if (WITH_A1) a1 = W.b1;
#pragma unroll
  for (int i4 = 0; i4 < 16; ++i4) {
    float4 w1v;
    if (WITH_A1) w1v = *reinterpret_cast<const float4*>(w1row + 4 * i4);
    const float w1a[4] = {w1v.x, w1v.y, w1v.z, w1v.w};
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int i = 4 * i4 + q;
      const float hi = rl(h, i);
      if (WITH_GH) {
        gh[0] = fmaf(W.whh[0][i], hi, gh[0]);
        gh[1] = fmaf(W.whh[1][i], hi, gh[1]);
        gh[2] = fmaf(W.whh[2][i], hi, gh[2]);
      }
      if (WITH_A1) a1 = fmaf(w1a[q], hi, a1);
    }
  }
}

// lane i <- sum over lanes j of ( W1[m_j][i]*da1h_j + W_hh[.*64+j][i] . (dpr,dpz,dghn)_j )
__device__ __forceinline__ float transposed_matvec(const FlowRegs& W, const float* w1row, float da1h, float dpr,
                                                   float dpz, float dghn, int lane) {
  float v[32];
#pragma unroll
  for (int i4 = 0; i4 < 8; ++i4) {
    const float4 wa = *reinterpret_cast<const float4*>(w1row + 4 * i4);
    const float4 wb = *reinterpret_cast<const float4*>(w1row + 32 + 4 * i4);
    const float a4[4] = {wa.x, wa.y, wa.z, wa.w};
    const float b4[4] = {wb.x, wb.y, wb.z, wb.w};
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int i = 4 * i4 + q;
      float lo = a4[q] * da1h;
      lo = fmaf(W.whh[0][i], dpr, lo);
      lo = fmaf(W.whh[1][i], dpz, lo);
      lo = fmaf(W.whh[2][i], dghn, lo);
      float hi = b4[q] * da1h;
      hi = fmaf(W.whh[0][i + 32], dpr, hi);
      hi = fmaf(W.whh[1][i + 32], dpz, hi);
      hi = fmaf(W.whh[2][i + 32], dghn, hi);
      v[i] = rs32(lo, hi);
    }
  }
#pragma unroll
  for (int i = 0; i < 16; ++i) v[i] = rs16(v[i], v[i + 16]);
#pragma unroll
  for (int i = 0; i < 8; ++i) v[i] = rs_small<8>(v[i], v[i + 8], lane);
#pragma unroll
  for (int i = 0; i < 4; ++i) v[i] = rs_small<4>(v[i], v[i + 4], lane);
#pragma unroll
  for (int i = 0; i < 2; ++i) v[i] = rs_small<2>(v[i], v[i + 2], lane);
  return rs_small<1>(v[0], v[1], lane);
}

__device__ __forceinline__ void head_finish(const FlowRegs& W, float a1, float& o0, float& o1, float& o2, float& o3) {
  // head layer 2: lanes <32 own outputs 0,1 (dloc); lanes >=32 own outputs 2,3 (scale)
  const float a = fmaxf(a1, 0.f);
  const float p0 = row_sum16(W.w2a * a);
  const float p1 = row_sum16(W.w2b * a);
  o0 = (rl(p0, 0) + rl(p0, 16)) + W.b2[0];
  o1 = (rl(p1, 0) + rl(p1, 16)) + W.b2[1];
  o2 = (rl(p0, 32) + rl(p0, 48)) + W.b2[2];
  o3 = (rl(p1, 32) + rl(p1, 48)) + W.b2[3];
}

// GRUCell adjoint of one step (gate order r, z, n), dh = dL/dh_{t+1}, tape (hprev, r, zg, n, ghn) of that step.
// Out: the pre-activation gradients dpr, dpz, dpn (= d gi_n), dghn = d gh_n, and the direct path dhdir = dL/dh_t via z*h.
__device__ __forceinline__ void gru_adjoint(float dh, float hprev, float r, float zg, float n, float ghn, float& dhdir,
                                            float& dpr, float& dpz, float& dpn, float& dghn) {
  const float dn = dh * (1.0f - zg);
  const float dzg = dh * (hprev - n);
  dhdir = dh * zg;
  dpn = dn * (1.0f - n * n);
  const float dr = dpn * ghn;
  dghn = dpn * r;
  dpr = dr * r * (1.0f - r);
  dpz = dzg * zg * (1.0f - zg);
}

}  // namespace

}  // namespace rip
