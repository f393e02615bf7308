// rip_load_model's host packers on the device (weights_pack.h): one member's packed parameter vector -> the eight weight
// buffers of a handle slot, in four launches on a stream.
//
//   zero_slot_kernel     the host fills every buffer from zero-initialised vectors (alignment padding of the blob, K-block
//                        padding of the operand fragments, the unused tails of the fp32 records, rows of the split blob
//                        nothing writes): the slot held another model before, so all of it is zeroed first
//   fold_kernel          fold_and_pack's encoder half: BatchNorm folded in double, the three re-layouts, the classifier /
//                        merger copies; writes the fp32 blob, its bf16 copy and the copy with bf16-valued depthwise taps
//   pack_flow_kernel     fold_and_pack's flow half and pack_split_operands: flow_w, mfma_w, split_w, and max |w|
//   pack_operands_kernel pack_split_tiles and pack_split_rows, gathered per output half from the folded blob
//
// Every kernel is a transcription of the host loop it replaces: a scatter where the host scatters (one work item per
// loop body, the loop variables decoded from the item), a gather where the host writes its output in order.  The
// arithmetic is the host's, operation for operation: nothing may contract (a fused multiply-add rounds once where the
// host rounds twice), which the pragma below and the __d*_rn intrinsics of the fold make sure of.  Double *, /, sqrt and
// the float / binary16 conversions are correctly rounded on both sides.
#include "weights_pack.h"

#include <hip/hip_runtime.h>

#include "flow.h"

#pragma clang fp contract(off)

namespace rip {
namespace {

constexpr double PK_BN_EPS = 1e-5;       // encoder.hip: BN_EPS
constexpr float PK_LO_SCALE = 2048.0f;   // flow_split_pack.h: SPLIT_LO_SCALE
constexpr float PK_TW_SCALE = 256.0f;    // flow_split_pack.h: SPLIT_TW_SCALE
// encoder_split_tile.hip: hidden channels per chunk record; features.18's records (build_pack_plan checks the layouts
// these give against the plan's)
constexpr int PK_HC = 64;
constexpr int PK_HD_CIN = 320, PK_HD_COUT = 1280, PK_HD_CH = 32, PK_HD_KS = PK_HD_CIN / 32;
constexpr int PK_HD_NF = (PK_HD_CH / 16) * PK_HD_KS * 2, PK_HD_REC = PK_HD_NF + 1, PK_HD_NCH = PK_HD_COUT / PK_HD_CH;

__device__ __forceinline__ unsigned short bf16_rne(float v) {  // rip_load_model's integer round to nearest even
  const unsigned u = __float_as_uint(v);
  return (unsigned short)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}
// float -> binary16, round to nearest even.  The value goes through an empty asm first: the backend otherwise selects
// f16(a * b) as ONE mixed-precision fused multiply-add with a +0 addend, and (-0) * b + (+0) is +0 where the host's
// product keeps the sign of a zero weight (the single rounding is harmless for the power-of-two scales used here; the
// lost sign is a different bit pattern in hi and, through v - hi, in lo).
__device__ __forceinline__ _Float16 to_f16(float v) {
  asm volatile("" : "+v"(v));
  return (_Float16)v;
}
__device__ __forceinline__ unsigned short f16_bits(float v) { return __builtin_bit_cast(unsigned short, to_f16(v)); }

// ---- zero ----
struct ZeroArgs {
  uint32_t* p[9];
  unsigned long long n[9];  // dwords
};
__global__ __launch_bounds__(256) void zero_slot_kernel(ZeroArgs a) {
  const size_t stride = (size_t)gridDim.x * blockDim.x;
#pragma unroll 1
  for (int r = 0; r < 9; ++r)
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.n[r]; i += stride) a.p[r][i] = 0u;
}

// ---- fold ----
__global__ __launch_bounds__(256) void fold_kernel(FoldPlan fp, const float* __restrict__ packed, float* __restrict__ enc,
                                                   unsigned short* __restrict__ enc_h, float* __restrict__ enc_t,
                                                   unsigned* __restrict__ flags) {
  const unsigned total = fp.start[fp.n_seg];
  const unsigned stride = gridDim.x * blockDim.x;
  int out_of_range = 0;
  for (unsigned item = blockIdx.x * blockDim.x + threadIdx.x; item < total; item += stride) {
    int lo = 0, hi = fp.n_seg - 1;  // the segment of this item: the last one that starts at or before it
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (fp.start[mid] <= item) lo = mid; else hi = mid - 1;
    }
    const FoldSeg& sg = fp.seg[lo];
    const unsigned idx = item - fp.start[lo];
    const float* w = packed + sg.src;
    float v;
    size_t dst;
    bool tap = false;
    if (sg.kind == PK_COPY) {
      v = w[idx];
      dst = (size_t)sg.w_off + idx;
    } else {
      const float* gamma = w + sg.wn;
      const float* beta = gamma + sg.cout;
      const float* mean = beta + sg.cout;
      const float* var = mean + sg.cout;
      const unsigned oc = idx < sg.wn ? idx / sg.per_out : idx - sg.wn;
      const double scale = __ddiv_rn((double)gamma[oc], __dsqrt_rn(__dadd_rn((double)var[oc], PK_BN_EPS)));
      if (idx >= sg.wn) {
        v = (float)__dsub_rn((double)beta[oc], __dmul_rn((double)mean[oc], scale));
        dst = (size_t)sg.b_off + oc;
      } else {
        const unsigned i = idx - oc * sg.per_out;
        v = (float)__dmul_rn((double)w[idx], scale);
        if (sg.kind == L_STEM) {  // reference [oc][c][ky][kx] -> [tap][c][oc]
          const unsigned c = i / 9, t = i - c * 9;
          dst = (size_t)sg.w_off + ((size_t)t * sg.cin + c) * sg.cout + oc;
        } else if (sg.kind == L_DW) {  // [oc][1][ky][kx] -> [tap][oc]
          dst = (size_t)sg.w_off + (size_t)i * sg.cout + oc;
          tap = true;
        } else {  // [oc][cin] kept
          dst = (size_t)sg.w_off + (size_t)oc * sg.cin + i;
          if (!(fabsf(v) < SPLIT_ENC_W_LIMIT)) out_of_range = 1;  // (true for NaN)
        }
      }
    }
    enc[dst] = v;
    const unsigned short h = bf16_rne(v);
    enc_h[dst] = h;
    enc_t[dst] = tap ? __uint_as_float((unsigned)h << 16) : v;
  }
  if (__syncthreads_or(out_of_range) && threadIdx.x == 0) atomicOr(&flags[2], 1u);
}

// ---- flow ----
// One wave per task, lane = the host loops' `lane` / `j`; the tasks are the bodies of the host loops one level above.
enum {
  T_FW_WHH = 0,                  // 48: chunk c = g * 16 + i4
  T_FW_MISC = T_FW_WHH + 48,     // 1
  T_FW_W1 = T_FW_MISC + 1,       // 32: row of W1
  T_MW_WHH = T_FW_W1 + 32,       // 12: (g, up)
  T_MW_IN = T_MW_WHH + 12,       // 1
  T_MW_HEAD = T_MW_IN + 1,       // 1
  T_MW_BW1 = T_MW_HEAD + 1,      // 1
  T_MW_BWHH = T_MW_BW1 + 1,      // 12: (g, up)
  T_MH_WHH = T_MW_BWHH + 12,     // 24: (g, up, kb)
  T_MH_W1 = T_MH_WHH + 24,       // 4: (mt, kb)
  T_MH_W1T = T_MH_W1 + 4,        // 4: ut
  T_MH_WHHT = T_MH_W1T + 4,      // 24: (kb, ut)
  T_MH_KS = T_MH_WHHT + 24,      // 12: (g, up)
  T_MH_IMG = T_MH_KS + 12,       // 1
  T_MH_TAB = T_MH_IMG + 1,       // 1
  T_SCAN_A = T_MH_TAB + 1,       // 198: 64 elements each of (W_ih, W_hh), contiguous in the packed vector
  T_SCAN_B = T_SCAN_A + 198,     // 32: ... of W1
  T_COUNT = T_SCAN_B + 32,
};
static_assert((192 * 2 + 192 * 64) == 198 * 64 && 32 * 64 == 32 * 64, "scan tasks");

struct FlowOut {
  float* flow;
  float* mw;
  uint32_t* mh;
  unsigned short* mh16;  // the same memory as halves: half i of dword d is mh16[2 d + i] (little endian)
};
__device__ __forceinline__ void put_h(const FlowOut& o, size_t row_base_dw, int lane, int i, unsigned short v) {
  o.mh16[(row_base_dw + (size_t)lane * 4 + (i >> 1)) * 2 + (i & 1)] = v;
}
// hi row at row_hi, lo' (forward rows) / lo (transposed rows) right behind it
__device__ __forceinline__ void put2(const FlowOut& o, int row_hi, int lane, int i, float w) {
  unsigned short h, l;
  if (row_hi >= MHF_ROWS) {
    const float ws = w * PK_TW_SCALE;
    const _Float16 hh = to_f16(ws);
    h = f16_bits((float)hh);
    l = f16_bits(ws - (float)hh);
  } else {
    const _Float16 hh = to_f16(w);
    const float r = (w - (float)hh) * PK_LO_SCALE;
    h = f16_bits((float)hh);
    l = f16_bits(r);
  }
  put_h(o, (size_t)row_hi * 256, lane, i, h);
  put_h(o, (size_t)(row_hi + 1) * 256, lane, i, l);
}
__device__ __forceinline__ void split3(float v, unsigned short t[3]) {
  const _Float16 h = to_f16(v);
  const float r1 = (v - (float)h) * PK_LO_SCALE;
  const _Float16 m = to_f16(r1);
  const float r2 = (r1 - (float)m) * PK_LO_SCALE;
  t[0] = f16_bits((float)h);
  t[1] = f16_bits((float)m);
  t[2] = f16_bits(r2);
}
// value idx of lane `lane` in the MW order; rows 48..51 and 60..62 are shared with the split blob
__device__ __forceinline__ void put_f(const FlowOut& o, int idx, int lane, float v) {
  const int row = idx >> 2;
  const size_t at = (size_t)row * 256 + lane * 4 + (idx & 3);
  o.mw[at] = v;
  if ((row >= MHF_WX && row < MHF_W1) || (row >= MHF_TAIL && row < MHF_BASE_ROWS)) o.mh[at] = __float_as_uint(v);
}
__device__ __forceinline__ void put_bk(const FlowOut& o, int f4, int lane, int comp, float v) {
  o.mw[MWF_FLOATS + ((size_t)f4 * 64 + lane) * 4 + comp] = v;
  if (f4 == 0) o.mh[(size_t)(MHF_ROWS + MHT_W2T) * 256 + lane * 4 + comp] = __float_as_uint(v);
}
__device__ __forceinline__ int unit_of(int kb, int i, int q) { return 16 * (2 * kb + (i >> 2)) + 4 * q + (i & 3); }
__device__ __forceinline__ int gate_row(int s, int q) { return (s >> 4) * 64 + 16 * ((s >> 2) & 3) + 4 * q + (s & 3); }

__global__ __launch_bounds__(64) void pack_flow_kernel(const float* __restrict__ fl, FlowOut o, unsigned* __restrict__ flags) {
  const float* wih = fl;
  const float* whh = wih + 192 * 2;
  const float* bih = whh + 192 * 64;
  const float* bhh = bih + 192;
  const float* w1 = bhh + 192;
  const float* b1 = w1 + 32 * 64;
  const float* w2 = b1 + 32;
  const float* b2 = w2 + 4 * 32;
  const int task = blockIdx.x, lane = threadIdx.x;
  const int m = lane & 15, q = lane >> 4;
  if (task < T_FW_MISC) {
    const int c = task - T_FW_WHH, g = c >> 4, i4 = c & 15, j = lane;
    for (int r = 0; r < 4; ++r) o.flow[FW_WHH + ((size_t)c * 64 + j) * 4 + r] = whh[(size_t)(g * 64 + j) * 64 + 4 * i4 + r];
  } else if (task < T_FW_W1) {
    const int j = lane;
    for (int g = 0; g < 3; ++g) {
      o.flow[FW_WIH + (g * 2 + 0) * 64 + j] = wih[(g * 64 + j) * 2 + 0];
      o.flow[FW_WIH + (g * 2 + 1) * 64 + j] = wih[(g * 64 + j) * 2 + 1];
      o.flow[FW_BIH + g * 64 + j] = bih[g * 64 + j];
      o.flow[FW_BHH + g * 64 + j] = bhh[g * 64 + j];
    }
    o.flow[FW_B1 + j] = b1[j & 31];
    o.flow[FW_W2 + j] = w2[(2 * (j >> 5) + 0) * 32 + (j & 31)];
    o.flow[FW_W2 + 64 + j] = w2[(2 * (j >> 5) + 1) * 32 + (j & 31)];
    if (j < 4) o.flow[FW_B2 + j] = b2[j];
  } else if (task < T_MW_WHH) {
    const int r = task - T_FW_W1;
    o.flow[FW_W1 + r * 64 + lane] = w1[r * 64 + lane];
  } else if (task < T_MW_IN) {
    const int gu = task - T_MW_WHH, g = gu >> 2, up = gu & 3;
    for (int u = 0; u < 4; ++u)
      for (int r = 0; r < 4; ++r)
        put_f(o, (g * 4 + up) * 16 + u * 4 + r, lane, whh[(size_t)(g * 64 + 16 * up + m) * 64 + 16 * u + 4 * q + r]);
  } else if (task < T_MW_HEAD) {
    for (int up = 0; up < 4; ++up) {
      const int j = 16 * up + m;
      for (int a = 0; a < 4; ++a) {
        const int g = a < 2 ? a : 2;
        float v = 0.f;
        if (a < 3) {
          if (q < 2) v = wih[(g * 64 + j) * 2 + q];
          if (q == 2) v = a < 2 ? bih[g * 64 + j] + bhh[g * 64 + j] : bih[g * 64 + j];
        } else if (q == 2) {
          v = bhh[128 + j];
        }
        put_f(o, 192 + a * 4 + up, lane, v);
      }
    }
  } else if (task < T_MW_BW1) {
    for (int mt = 0; mt < 2; ++mt) {
      for (int u = 0; u < 4; ++u)
        for (int r = 0; r < 4; ++r) put_f(o, 208 + mt * 16 + u * 4 + r, lane, w1[(16 * mt + m) * 64 + 16 * u + 4 * q + r]);
      put_f(o, 240 + mt, lane, q == 2 ? b1[16 * mt + m] : 0.f);
      for (int r = 0; r < 4; ++r) put_f(o, 242 + mt * 4 + r, lane, w2[(m & 3) * 32 + 16 * mt + 4 * q + r]);
    }
    put_f(o, 250, lane, q == 2 ? b2[m & 3] : 0.f);
    put_bk(o, 0, lane, 0, w2[q * 32 + m]);
    put_bk(o, 0, lane, 1, w2[q * 32 + 16 + m]);
  } else if (task < T_MW_BWHH) {
    for (int mt = 0; mt < 2; ++mt)
      for (int r = 0; r < 4; ++r)
        for (int ut = 0; ut < 4; ++ut) put_bk(o, 1 + mt * 4 + r, lane, ut, w1[(16 * mt + 4 * q + r) * 64 + 16 * ut + m]);
  } else if (task < T_MH_WHH) {
    const int gu = task - T_MW_BWHH, g = gu >> 2, up = gu & 3;
    for (int r = 0; r < 4; ++r) {
      const int s = (g * 4 + up) * 4 + r;
      const int j = g * 64 + 16 * up + 4 * q + r;
      for (int ut = 0; ut < 4; ++ut) put_bk(o, 9 + s, lane, ut, whh[(size_t)j * 64 + 16 * ut + m]);
      put_bk(o, 57 + s / 4, lane, s & 3, wih[j * 2 + (m & 1)]);
    }
  } else if (task < T_MH_W1) {  // ---- split blob, forward rows ----
    const int t = task - T_MH_WHH, kb = t & 1, up = (t >> 1) & 3, g = t >> 3;
    for (int i = 0; i < 8; ++i)
      put2(o, MHF_WHH + ((g * 4 + up) * 2 + kb) * 2, lane, i, whh[(size_t)(g * 64 + 16 * up + m) * 64 + unit_of(kb, i, q)]);
  } else if (task < T_MH_W1T) {
    const int t = task - T_MH_W1, kb = t & 1, mt = t >> 1;
    for (int i = 0; i < 8; ++i) put2(o, MHF_W1 + (mt * 2 + kb) * 2, lane, i, w1[(16 * mt + m) * 64 + unit_of(kb, i, q)]);
  } else if (task < T_MH_WHHT) {  // ---- transposed rows ----
    const int ut = task - T_MH_W1T;
    for (int i = 0; i < 8; ++i) put2(o, MHF_ROWS + MHT_W1T + ut * 2, lane, i, w1[(16 * (i >> 2) + 4 * q + (i & 3)) * 64 + 16 * ut + m]);
  } else if (task < T_MH_KS) {
    const int t = task - T_MH_WHHT, ut = t & 3, kb = t >> 2;
    for (int i = 0; i < 8; ++i)
      put2(o, MHF_ROWS + MHT_WHHT + (kb * 4 + ut) * 2, lane, i, whh[(size_t)gate_row(8 * kb + i, q) * 64 + 16 * ut + m]);
  } else if (task < T_MH_IMG) {  // ---- the input / bias k-steps as one f16 K block per (gate, unit tile) ----
    const int gu = task - T_MH_KS, g = gu >> 2, up = gu & 3;
    const int j = 16 * up + m;
    unsigned short k[16];
    for (int i = 0; i < 16; ++i) k[i] = 0;
    for (int d = 0; d < 2; ++d) {
      unsigned short t[3];
      split3(4.0f * wih[(g * 64 + j) * 2 + d], t);
      k[6 * d + 0] = t[0], k[6 * d + 1] = t[0], k[6 * d + 2] = t[0], k[6 * d + 3] = t[1], k[6 * d + 4] = t[1], k[6 * d + 5] = t[2];
    }
    unsigned short t[3];
    split3(g < 2 ? bih[g * 64 + j] + bhh[g * 64 + j] : bih[g * 64 + j], t);
    k[12] = t[0], k[13] = t[1], k[14] = t[2];
    if (q < 2)
      for (int i = 0; i < 8; ++i) put_h(o, (size_t)(MHF_KS + g * 4 + up) * 256, lane, i, q == 0 ? k[i] : k[8 + i]);
  } else if (task < T_MH_TAB) {  // ---- accumulator images, W2 x 4, b2 ----
    for (int up = 0; up < 4; ++up)
      for (int r = 0; r < 4; ++r) o.mh[(size_t)(MHF_GHB + up) * 256 + lane * 4 + r] = __float_as_uint(bhh[128 + 16 * up + 4 * q + r]);
    for (int mt = 0; mt < 2; ++mt)
      for (int r = 0; r < 4; ++r) o.mh[(size_t)(MHF_B1 + mt) * 256 + lane * 4 + r] = __float_as_uint(b1[16 * mt + 4 * q + r]);
    for (int i = 0; i < 8; ++i) {
      const int unit = i < 4 ? 4 * q + i : 16 + 4 * q + (i - 4);
      put2(o, MHF_W2, lane, i, 4.0f * w2[(m & 3) * 32 + unit]);  // (a forward row: hi, lo')
    }
    for (int r = 0; r < 4; ++r) o.mh[(size_t)MHF_B2 * 256 + lane * 4 + r] = __float_as_uint(b2[r]);
  } else if (task < T_SCAN_A) {  // ---- W_ih^T table: entry ((kb * 2 + term) * 8 + q * 2 + parity), 8 halves each ----
    const size_t tab = (size_t)(MHF_ROWS + MHT_ROWS) * 256;
    for (int it = lane; it < 6 * 4 * 2 * 8; it += 64) {
      const int i = it & 7, par = (it >> 3) & 1, tq = (it >> 4) & 3, kb = it >> 6;
      const float ws = wih[gate_row(8 * kb + i, tq) * 2 + par] * PK_TW_SCALE;
      const _Float16 hh = to_f16(ws);
      const size_t e_hi = tab + (size_t)((kb * 2 + 0) * 8 + tq * 2 + par) * 4;
      const size_t e_lo = tab + (size_t)((kb * 2 + 1) * 8 + tq * 2 + par) * 4;
      o.mh16[(e_hi + (i >> 1)) * 2 + (i & 1)] = f16_bits((float)hh);
      o.mh16[(e_lo + (i >> 1)) * 2 + (i & 1)] = f16_bits(ws - (float)hh);
    }
  } else {  // ---- max |w| over W_ih, W_hh, W1; a NaN / infinite weight is tracked on its own, as the host does ----
    const float* base = task < T_SCAN_B ? wih + (size_t)(task - T_SCAN_A) * 64 : w1 + (size_t)(task - T_SCAN_B) * 64;
    float a = fabsf(base[lane]);
    const bool bad = !(a <= 3.402823466e38f);
    if (bad) a = 0.f;
    for (int sh = 32; sh >= 1; sh >>= 1) {
      const float other = __shfl_xor(a, sh, 64);
      a = other > a ? other : a;
    }
    const unsigned long long any_bad = __ballot(bad);
    if (lane == 0) {
      atomicMax(&flags[0], __float_as_uint(a));  // (non-negative floats order as their bit patterns)
      if (any_bad != 0ull) atomicOr(&flags[1], 1u);
    }
  }
}

// ---- encoder operands ----
// w * 2^8 as hi = f16(.), lo = f16(. - hi)  (pack_split_tiles / pack_split_rows: `put`)
__device__ __forceinline__ unsigned short enc_term(float wv, int term) {
  const float v = wv * SPLIT_ENC_W_SCALE;
  const _Float16 hi = to_f16(v);
  const _Float16 lo = to_f16(v - (float)hi);
  return __builtin_bit_cast(unsigned short, term ? lo : hi);
}
__device__ __forceinline__ unsigned short f32_half(float v, unsigned which) { return (unsigned short)(__float_as_uint(v) >> (16 * which)); }

__global__ __launch_bounds__(256) void pack_operands_kernel(OperandPlan op, const float* __restrict__ enc,
                                                            unsigned short* __restrict__ wc, unsigned short* __restrict__ wr) {
  const unsigned total = op.tiles_total + op.rows_total;
  const unsigned stride = gridDim.x * blockDim.x;
  for (unsigned o = blockIdx.x * blockDim.x + threadIdx.x; o < total; o += stride) {
    if (o < op.tiles_total) {
      if (op.has_head && o >= op.head_off) {
        // features.18: chunk c = output channels 32 c ..: fragments (ht, ks, term), then 1 KB with the 32 biases
        const unsigned r = o - op.head_off, c = r / (PK_HD_REC * 512), e = r - c * (PK_HD_REC * 512), piece = e >> 9;
        if (piece < (unsigned)PK_HD_NF) {
          const unsigned term = piece & 1, ks = (piece >> 1) % PK_HD_KS, ht = (piece >> 1) / PK_HD_KS, lane = (e >> 3) & 63, j = e & 7;
          wc[o] = enc_term(enc[op.head_w_off + (size_t)(c * PK_HD_CH + 16 * ht + (lane & 15)) * PK_HD_CIN + 32 * ks + 8 * (lane >> 4) + j], term);
        } else {
          const unsigned t = e - PK_HD_NF * 512, fi = t >> 1;
          wc[o] = fi < (unsigned)PK_HD_CH ? f32_half(enc[op.head_b_off + c * PK_HD_CH + fi], t & 1) : (unsigned short)0;
        }
        continue;
      }
      int b = 0;
      while (b + 1 < op.n_tile && op.tile[b + 1].off <= o) ++b;
      const TileBlk& tb = op.tile[b];
      const unsigned r = o - tb.off, c = r / tb.rec, e = r - c * tb.rec, piece = e >> 9, lane = (e >> 3) & 63, j = e & 7;
      if (piece < tb.nfe) {  // expansion fragments (ht, ks, term)
        const unsigned term = piece & 1, ks = (piece >> 1) % tb.ksx, ht = (piece >> 1) / tb.ksx;
        wc[o] = enc_term(enc[tb.we_off + (size_t)(c * PK_HC + 16 * ht + (lane & 15)) * tb.cin + 32 * ks + 8 * (lane >> 4) + j], term);
      } else if (piece < tb.nfe + tb.nfp) {  // projection fragments (ct, ks, term)
        const unsigned p = piece - tb.nfe, term = p & 1, ks = (p >> 1) % (PK_HC / 32), ct = (p >> 1) / (PK_HC / 32);
        wc[o] = enc_term(enc[tb.wp_off + (size_t)(16 * ct + (lane & 15)) * tb.hid + c * PK_HC + 32 * ks + 8 * (lane >> 4) + j], term);
      } else {  // 3 KB of fp32: depthwise taps [9][64], depthwise biases [64], expansion biases [64], zeros
        const unsigned t = e - (tb.nfe + tb.nfp) * 512, fi = t >> 1, row = fi / PK_HC, i = fi - row * PK_HC;
        float v = 0.f;
        if (row < 9) v = enc[tb.wd_off + (size_t)row * tb.hid + c * PK_HC + i];
        else if (row == 9) v = enc[tb.bd_off + c * PK_HC + i];
        else if (row == 10) v = enc[tb.be_off + c * PK_HC + i];
        wc[o] = f32_half(v, t & 1);
      }
    } else {
      const unsigned ro = o - op.tiles_total;
      int b = 0;
      while (b + 1 < op.n_rows && op.rows[b + 1].off <= ro) ++b;
      const RowsBlk& rb = op.rows[b];
      const unsigned e = ro - rb.off, piece = e >> 9, lane = (e >> 3) & 63, j = e & 7;
      float w = 0.f;
      unsigned term;
      if (piece < rb.nfe) {  // expansion fragment (ct, term)
        term = piece & 1;
        const unsigned ct = piece >> 1, row = 16 * ct + (lane & 15), kk = 8 * (lane >> 4) + j;
        if (kk < rb.cin) w = enc[rb.we_off + (size_t)row * rb.cin + kk];
      } else {  // projection fragment (ct, ks, term)
        const unsigned p = piece - rb.nfe;
        term = p & 1;
        const unsigned ks = (p >> 1) % rb.nkp, ct = (p >> 1) / rb.nkp, row = 16 * ct + (lane & 15), kk = 32 * ks + 8 * (lane >> 4) + j;
        if (row < rb.cout && kk < rb.hid) w = enc[rb.wp_off + (size_t)row * rb.hid + kk];
      }
      wr[ro] = enc_term(w, (int)term);
    }
  }
}

}  // namespace

PackPlan build_pack_plan(const EncoderPlan& plan) {
  PackPlan pp;
  FoldPlan& fp = pp.fold;
  size_t pos = 0, items = 0;
  auto seg = [&](const FoldSeg& s, size_t n_items, size_t n_floats) {
    if (fp.n_seg >= PK_MAX_SEG) return false;
    fp.start[fp.n_seg] = (unsigned)items;
    fp.seg[fp.n_seg++] = s;
    items += n_items;
    pos += n_floats;
    return true;
  };
  bool ok = true;
  for (const Layer& l : plan.layers) {
    FoldSeg s = {};
    s.per_out = l.kind == L_STEM ? (unsigned)l.cin * 9 : (l.kind == L_DW ? 9u : (unsigned)l.cin);
    s.wn = s.per_out * (unsigned)l.cout;
    s.src = (unsigned)pos;
    s.cin = (unsigned)l.cin;
    s.cout = (unsigned)l.cout;
    s.kind = (unsigned)l.kind;
    s.w_off = (unsigned)l.w_off;
    s.b_off = (unsigned)l.b_off;
    ok = ok && seg(s, (size_t)s.wn + l.cout, (size_t)s.wn + 4 * (size_t)l.cout);
  }
  auto copy = [&](size_t dst, size_t n) {
    FoldSeg s = {};
    s.src = (unsigned)pos;
    s.wn = (unsigned)n;
    s.kind = PK_COPY;
    s.w_off = (unsigned)dst;
    ok = ok && seg(s, n, n);
  };
  constexpr int FEAT = 128, LAST_C = 1280, VEC = 5, HID = 64;  // encoder.hip (classifier.1 [128][1280], merger 133 -> 64 -> 64 -> 64)
  copy(plan.cls_w_off, (size_t)FEAT * LAST_C);
  copy(plan.cls_b_off, FEAT);
  const int sizes[4] = {FEAT + VEC, HID, HID, HID};
  for (int i = 0; i < 3; ++i) {
    copy(plan.mrg_w_off[i], (size_t)sizes[i + 1] * sizes[i]);
    copy(plan.mrg_b_off[i], sizes[i + 1]);
  }
  if (!ok) return pp;
  fp.start[fp.n_seg] = (unsigned)items;
  pp.flow_pos = pos;
  pp.numel = pos + 192 * 2 + 192 * 64 + 192 + 192 + 32 * 64 + 32 + 4 * 32 + 4;
  // the last merger bias ends the blob: the copies above must fit it exactly as fold_and_pack's do
  ok = plan.mrg_b_off[2] + HID <= plan.blob_floats && pp.numel < (1ull << 31) && plan.blob_floats < (1ull << 31);

  // ---- operand records: the layouts of split_tile_layout / split_rows_layout, re-derived and checked against them ----
  OperandPlan& op = pp.ops;
  size_t off = 0;
  for (size_t bi = 0; bi < plan.blocks.size(); ++bi) {
    if (plan.split_tiles.off[bi] == (size_t)-1) continue;
    const FusedBlock& fb = plan.blocks[bi];
    if (fb.expand < 0 || op.n_tile >= 12) return pp;
    const Layer &le = plan.layers[fb.expand], &ld = plan.layers[fb.dw], &lp = plan.layers[fb.project];
    TileBlk& t = op.tile[op.n_tile++];
    t.cin = (unsigned)le.cin;
    t.hid = (unsigned)ld.cout;
    t.ksx = (unsigned)le.cin / 32;
    t.nfe = (PK_HC / 16) * t.ksx * 2;
    t.nfp = ((unsigned)lp.cout / 16) * (PK_HC / 32) * 2;
    t.rec = (t.nfe + t.nfp + 3) * 512;
    t.nch = t.hid / PK_HC;
    t.off = (unsigned)off;
    t.we_off = (unsigned)le.w_off;
    t.wp_off = (unsigned)lp.w_off;
    t.wd_off = (unsigned)ld.w_off;
    t.bd_off = (unsigned)ld.b_off;
    t.be_off = (unsigned)le.b_off;
    ok = ok && plan.split_tiles.off[bi] == off && le.cin % 32 == 0 && lp.cout % 16 == 0 && ld.cout % PK_HC == 0;
    off += (size_t)t.rec * t.nch;
  }
  if (plan.split_tiles.head_off != (size_t)-1) {
    const Layer& l = plan.layers.back();
    op.has_head = 1;
    op.head_off = (unsigned)off;
    op.head_w_off = (unsigned)l.w_off;
    op.head_b_off = (unsigned)l.b_off;
    ok = ok && plan.split_tiles.head_off == off && l.cin == PK_HD_CIN && l.cout == PK_HD_COUT;
    off += (size_t)PK_HD_NCH * PK_HD_REC * 512;
  }
  ok = ok && off == plan.split_tiles.total && op.n_tile >= 1;
  op.tiles_total = (unsigned)off;
  off = 0;
  for (size_t bi = 0; bi < plan.blocks.size(); ++bi) {
    if (plan.split_rows.off[bi] == (size_t)-1) continue;
    const FusedBlock& fb = plan.blocks[bi];
    if (op.n_rows >= 8) return pp;
    const Layer &ld = plan.layers[fb.dw], &lp = plan.layers[fb.project];
    const Layer& le = plan.layers[fb.expand >= 0 ? fb.expand : fb.dw];
    RowsBlk& r = op.rows[op.n_rows++];
    r.cin = (unsigned)le.cin;
    r.hid = (unsigned)ld.cout;
    r.cout = (unsigned)lp.cout;
    r.nfe = fb.expand >= 0 ? r.hid / 16 * 2 : 0;
    r.nkp = (r.hid + 31) / 32;
    r.n = (r.nfe + ((r.cout + 15) / 16) * r.nkp * 2) * 512;
    r.off = (unsigned)off;
    r.we_off = (unsigned)le.w_off;
    r.wp_off = (unsigned)lp.w_off;
    ok = ok && plan.split_rows.off[bi] == off && (fb.expand < 0 || r.hid % 16 == 0);
    off += r.n;
  }
  ok = ok && off == plan.split_rows.total && op.n_rows >= 1;
  op.rows_total = (unsigned)off;
  ok = ok && (size_t)op.tiles_total + op.rows_total < (1ull << 31);
  pp.ok = ok;
  return pp;
}

hipError_t launch_pack_weights(const EncoderPlan& plan, const PackPlan& pp, const float* packed_dev, const PackTargets& t,
                               hipStream_t s) {
  if (!pp.ok) return hipErrorInvalidValue;
  ZeroArgs z;
  z.p[0] = reinterpret_cast<uint32_t*>(t.enc_w), z.n[0] = plan.blob_floats;
  z.p[1] = reinterpret_cast<uint32_t*>(t.enc_wh), z.n[1] = plan.blob_floats / 2;
  z.p[2] = reinterpret_cast<uint32_t*>(t.enc_wt), z.n[2] = plan.blob_floats;
  z.p[3] = reinterpret_cast<uint32_t*>(t.enc_wc), z.n[3] = plan.split_tiles.total / 2;
  z.p[4] = reinterpret_cast<uint32_t*>(t.enc_wr), z.n[4] = plan.split_rows.total / 2;
  z.p[5] = reinterpret_cast<uint32_t*>(t.flow_w), z.n[5] = FW_SIZE;
  z.p[6] = reinterpret_cast<uint32_t*>(t.mfma_w), z.n[6] = MW_SIZE;
  z.p[7] = t.split_w, z.n[7] = MH_SIZE;
  z.p[8] = t.flags, z.n[8] = 4;
  // (blob_floats is a multiple of 4 and the record totals are multiples of 512: every slot is whole, aligned dwords)
  if (plan.blob_floats % 2 != 0 || plan.split_tiles.total % 2 != 0 || plan.split_rows.total % 2 != 0) return hipErrorInvalidValue;
  hipLaunchKernelGGL(zero_slot_kernel, dim3(1024), dim3(256), 0, s, z);
  const unsigned fold_items = pp.fold.start[pp.fold.n_seg];
  hipLaunchKernelGGL(fold_kernel, dim3((fold_items + 255) / 256 < 2048 ? (fold_items + 255) / 256 : 2048), dim3(256), 0, s, pp.fold,
                     packed_dev, t.enc_w, t.enc_wh, t.enc_wt, t.flags);
  FlowOut fo;
  fo.flow = t.flow_w;
  fo.mw = t.mfma_w;
  fo.mh = t.split_w;
  fo.mh16 = reinterpret_cast<unsigned short*>(t.split_w);
  hipLaunchKernelGGL(pack_flow_kernel, dim3(T_COUNT), dim3(64), 0, s, packed_dev + pp.flow_pos, fo, t.flags);
  const unsigned halves = pp.ops.tiles_total + pp.ops.rows_total;
  hipLaunchKernelGGL(pack_operands_kernel, dim3((halves + 255) / 256 < 4096 ? (halves + 255) / 256 : 4096), dim3(256), 0, s, pp.ops,
                     t.enc_w, t.enc_wc, t.enc_wr);
  return hipGetLastError();
}

}  // namespace rip
