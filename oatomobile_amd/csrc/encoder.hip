// MobileNetV2 BEV encoder + merger for gfx950, BN folded, NHWC fp32 activations.
//
// Replaces the ATen work of ImitativeModel._params (oatomobile/baselines/torch/dim/model.py:173-219):
//   K1 transform          torch/transforms.py:34-49   -> transform_kernel
//   K2 stem 3x3 s2        perception.py:43-51 / torchvision features.0     -> stem_kernel
//   K3 depthwise 3x3      torchvision features.{1..17}.conv.*              -> dw_kernel (HBM-bound, float4/lane)
//   K4 pointwise 1x1      torchvision features.*.conv.*, features.18       -> pw_kernel (fp32-input MFMA 32x32x2)
//   K5/K6 pool+classifier+merger  dim/model.py:203-217                     -> tail_kernel
// All K ensemble members run in the same launches (blockIdx.z = model).
#include "encoder.h"
#include "flow_split_pack.h"
#include "flow.h"

#include <mutex>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>

namespace rip {

// ---- kernel-selection log (encoder.h) ----
static thread_local KernelLog* g_kernel_log = nullptr;
void kernel_log_install(KernelLog* log) { g_kernel_log = log; }
bool kernel_log_active() { return g_kernel_log != nullptr; }
void note_kernel(dim3 grid, dim3 block, const char* fmt, ...) {
  if (g_kernel_log == nullptr) return;
  char name[256], line[320];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(name, sizeof(name), fmt, ap);
  va_end(ap);
  snprintf(line, sizeof(line), "%s grid=(%u,%u,%u) block=%u\n", name, grid.x, grid.y, grid.z, block.x);
  g_kernel_log->text += line;
}

namespace {

constexpr int IR_SETTING[7][4] = {{1, 16, 1, 1}, {6, 24, 2, 2}, {6, 32, 3, 2}, {6, 64, 4, 2},
                                  {6, 96, 3, 1}, {6, 160, 3, 2}, {6, 320, 1, 1}};
constexpr int STEM_C = 32, LAST_C = 1280, FEAT = 128, VEC = 5, HID = 64, IN_HW = 100;
constexpr double BN_EPS = 1e-5;

inline int conv_out(int h, int stride) { return (h + 2 - 3) / stride + 1; }


__device__ __forceinline__ float relu6f(float v) { return fminf(fmaxf(v, 0.f), 6.f); }

// ------------------------------------------------------------------------------------------------
// K1: bilinear (H,W)->(O,O), align_corners=True, then swap H/W.  out[b][c][i][j] = interp[b][c][j][i].
// ATen computes scale=(in-1)/(out-1) and src=scale*dst in fp32 (UpSample.h area_pixel_compute_*).
// ------------------------------------------------------------------------------------------------
// ATen rounds scale*dst to fp32 before taking the fraction (UpSample.h area_pixel_compute_source_index); hipcc's
// default fp-contract=fast would fuse the product into the subtraction and change lambda by up to half an ulp of
// the coordinate (1e-5 at 199), so contraction is switched off for exactly this computation.
__device__ __forceinline__ void src_coord(float scale, int dst, int size, int& lo, int& hi, float& lambda) {
#pragma clang fp contract(off)
  const float f = scale * (float)dst;
  lo = (int)f;
  hi = lo + (lo < size - 1 ? 1 : 0);
  lambda = f - (float)lo;
}

__device__ __forceinline__ float bilerp_fetch(const float* __restrict__ in, int b, int c, int y, int x, int C, int H,
                                              int W, int channels_last) {
  return channels_last ? in[(((size_t)b * H + y) * W + x) * C + c] : in[(((size_t)b * C + c) * H + y) * W + x];
}

// Tiled through LDS: output (i, j) samples input row ~ j*scale and column ~ i*scale, so a naive thread-per-output
// mapping reads one input ROW per consecutive thread.  A block owns a TxT output tile, stages the matching input
// patch with coalesced row reads, then every thread interpolates from LDS and writes NCHW rows coalesced.
constexpr int TR_T = 32;            // output tile edge
constexpr int TR_P = 2 * TR_T + 4;  // input patch edge bound for scale <= 2.02 (200 -> 100)
// TIN = float: the sensor's float32 BEV.  TIN = uint8_t: a CODED BEV (replay cache, oatomobile_amd/replay.py): every
// cell holds an index into `lut` (256 float32 values, the distinct values of the float BEV it was packed from), looked
// up while the patch is staged — a quarter of the bytes, the same float32 values, hence bit-identical outputs.
// One TxT output tile (ti, tj) of ONE image: `in` points at the image, `out` at its [C,O,O] output, `patch` at the
// dynamic LDS (patch, then for TIN = uint8_t the 256-entry table).  Called by transform_kernel and gather_batch_kernel.
template <int C, bool CL, typename TIN>
__device__ __forceinline__ void transform_tile(const TIN* __restrict__ in, const float* __restrict__ lut, int H, int W,
                                               int O, float* __restrict__ out, int ti, int tj, float* patch) {
  // The patch keeps the memory order of the input; all staging loads of a thread are issued before the first LDS
  // write (the kernel is pure latency otherwise), and the row pitch is odd so the interpolation reads (consecutive
  // lanes sit two patch rows apart) spread over the banks.
  constexpr int ROW = CL ? TR_P * C : TR_P;
  constexpr int NROWS = CL ? TR_P : TR_P * C;
  constexpr int PITCH = ROW + 1;
  constexpr int TOTAL = ROW * NROWS;
  constexpr int ITER = (TOTAL + 255) / 256;
  constexpr bool CODED = sizeof(TIN) == 1;
  float* lut_s = patch + PITCH * NROWS;  // CODED: the table, behind the patch
  if (CODED) lut_s[threadIdx.x] = lut[threadIdx.x];
  const float sh = O > 1 ? (float)(H - 1) / (float)(O - 1) : 0.f;
  const float sw = O > 1 ? (float)(W - 1) / (float)(O - 1) : 0.f;
  // ti: output rows i (input x), tj: output cols j (input y)
  const int i0 = ti * TR_T, j0 = tj * TR_T;
  const int y0 = (int)(sh * (float)j0), x0 = (int)(sw * (float)i0);
  const int py = min(TR_P, H - y0), px = min(TR_P, W - x0);
  const int tid = threadIdx.x;
  TIN v[ITER];
#pragma unroll
  for (int k = 0; k < ITER; ++k) {
    const int e = tid + 256 * k, r = e / ROW, t = e - r * ROW;
    bool ok;
    const TIN* src;
    if (CL) {
      ok = r < py && t < px * C;
      src = in + ((size_t)(y0 + r) * W + x0) * C + t;
    } else {
      const int c = r / TR_P, y = r - c * TR_P;
      ok = c < C && y < py && t < px;
      src = in + ((size_t)c * H + y0 + y) * W + x0 + t;
    }
    v[k] = ok ? *src : (TIN)0;
  }
  if (CODED) __syncthreads();  // the table is in LDS
#pragma unroll
  for (int k = 0; k < ITER; ++k) {
    const int e = tid + 256 * k, r = e / ROW, t = e - r * ROW;
    if (e < TOTAL) {
      if constexpr (CODED) {
        const bool ok = CL ? (r < py && t < px * C) : ((r / TR_P) < C && (r % TR_P) < py && t < px);
        patch[r * PITCH + t] = ok ? lut_s[v[k]] : 0.f;  // cells outside the image stay 0, whatever code 0 means
      } else {
        patch[r * PITCH + t] = v[k];
      }
    }
  }
  __syncthreads();
  constexpr int XS = CL ? C : 1;  // element stride along x
#pragma unroll
  for (int k = 0; k < C * TR_T * TR_T / 256; ++k) {
    const int e = tid + 256 * k;
    const int jl = e % TR_T, il = (e / TR_T) % TR_T, c = e / (TR_T * TR_T);
    const int i = i0 + il, j = j0 + jl;
    if (i >= O || j >= O) continue;
    int ya, yb, xa, xb;
    float ly, lx;
    src_coord(sh, j, H, ya, yb, ly);
    src_coord(sw, i, W, xa, xb, lx);
    const float hy = 1.f - ly, hx = 1.f - lx;
    const float* pc = CL ? patch + c : patch + c * TR_P * PITCH;
    const float v00 = pc[(ya - y0) * PITCH + (xa - x0) * XS], v01 = pc[(ya - y0) * PITCH + (xb - x0) * XS];
    const float v10 = pc[(yb - y0) * PITCH + (xa - x0) * XS], v11 = pc[(yb - y0) * PITCH + (xb - x0) * XS];
    out[((size_t)c * O + i) * O + j] = hy * (hx * v00 + lx * v01) + ly * (hx * v10 + lx * v11);
  }
}

template <int C, bool CL, typename TIN = float>
__global__ __launch_bounds__(256) void transform_kernel(const TIN* __restrict__ in, const float* __restrict__ lut, int H,
                                                         int W, int O, float* __restrict__ out) {
  extern __shared__ float patch[];
  const size_t b = blockIdx.z;
  transform_tile<C, CL, TIN>(in + b * H * W * C, lut, H, W, O, out + b * C * O * O, blockIdx.y, blockIdx.x, patch);
}

// A trainer batch straight out of a device-resident coded cache (replay.DeviceCache): block (tj, ti, b) gathers row
// rows[b] of `codes` [n,H,W,C] and runs the coded tile above on it; the first tile of each row also gathers the row's
// vec [5], its target future[row, 0::stride][:T] (transforms.downsample_target) and, if asked, its CIL mode with
// STOP (1) rewritten to FORWARD (0) (cil/model.py:166-168).  Row offsets are 64-bit: 100 k observations of
// 200 x 200 x 2 codes are 8 GB.  A row outside [0, n) reads nothing and yields NaN outputs.
template <int C>
__global__ __launch_bounds__(256) void gather_batch_kernel(const uint8_t* __restrict__ codes, const float* __restrict__ lut,
                                                           const int64_t* __restrict__ rows, int64_t n, int H, int W, int O,
                                                           const float* __restrict__ vec, const float* __restrict__ future,
                                                           int L, int T, int stride, const float* __restrict__ mode,
                                                           float* __restrict__ visual, float* __restrict__ vec_out,
                                                           float* __restrict__ target, float* __restrict__ mode_out) {
  extern __shared__ float patch[];
  const int b = blockIdx.z;
  const int64_t row = rows[b];
  const bool valid = row >= 0 && row < n;
  const int tid = threadIdx.x;
  if (blockIdx.x == 0 && blockIdx.y == 0) {
    const float nan = __builtin_nanf("");
    if (tid < 5) vec_out[(size_t)b * 5 + tid] = valid ? vec[row * 5 + tid] : nan;
    for (int e = tid; e < 2 * T; e += 256) {
      const int t = e >> 1, d = e & 1;
      target[(size_t)b * 2 * T + e] = valid ? future[(row * L + (int64_t)t * stride) * 2 + d] : nan;
    }
    if (mode_out != nullptr && tid == 0) {
      const float m = valid ? mode[row] : nan;
      mode_out[b] = m == 1.f ? 0.f : m;
    }
  }
  float* out = visual + (size_t)b * C * O * O;
  if (!valid) {  // uniform over the block
    const int i0 = blockIdx.y * TR_T, j0 = blockIdx.x * TR_T;
    for (int e = tid; e < C * TR_T * TR_T; e += 256) {
      const int jl = e % TR_T, il = (e / TR_T) % TR_T, c = e / (TR_T * TR_T);
      if (i0 + il < O && j0 + jl < O) out[((size_t)c * O + i0 + il) * O + j0 + jl] = __builtin_nanf("");
    }
    return;
  }
  transform_tile<C, true, uint8_t>(codes + row * H * W * C, lut, H, W, O, out, blockIdx.y, blockIdx.x, patch);
}

template <int C, bool CL, typename TIN = float>
void launch_transform_tiled(const TIN* in, const float* lut, int B, int H, int W, int O, float* out, hipStream_t s) {
  constexpr int ROW = CL ? TR_P * C : TR_P;
  constexpr int NROWS = CL ? TR_P : TR_P * C;
  const int tiles = (O + TR_T - 1) / TR_T;
  const size_t lds = ((size_t)(ROW + 1) * NROWS + (sizeof(TIN) == 1 ? 256 : 0)) * sizeof(float);
  hipLaunchKernelGGL((transform_kernel<C, CL, TIN>), dim3(tiles, tiles, B), dim3(256), lds, s, in, lut, H, W, O, out);
}

// The blend of the four neighbours with every rounding spelled out, in the order the compiler gives the tiled kernels'
// expression `hy * (hx * v00 + lx * v01) + ly * (hx * v10 + lx * v11)` under fp-contract=fast (one product of each row
// rounded, the other fused into it; the two row products rounded, then added).  Left to the compiler, the generic kernel
// fused the other product of a row: its outputs sat one ulp from the tiled kernels' on about one output in a thousand,
// and rip_gather_batch_u8 with C = 4 (tiled) was not "rip_transform(lut[codes[rows]]) bit for bit" (generic for C = 4)
// as include/rip_hip.h has it — found by tests/test_shapes.py.
__device__ __forceinline__ float bilerp_blend_as_tiled(float hy, float hx, float ly, float lx, float v00, float v01,
                                                       float v10, float v11) {
  const float top = fmaf(lx, v01, __fmul_rn(hx, v00));
  const float bot = fmaf(hx, v10, __fmul_rn(lx, v11));
  return __fadd_rn(__fmul_rn(hy, top), __fmul_rn(ly, bot));
}

// generic fallback (any scale): one thread per output element
__global__ void transform_generic_kernel(const float* __restrict__ in, int B, int C, int H, int W, int channels_last,
                                         int O, float* __restrict__ out) {
  const int total = B * C * O * O;
  const float sh = O > 1 ? (float)(H - 1) / (float)(O - 1) : 0.f;
  const float sw = O > 1 ? (float)(W - 1) / (float)(O - 1) : 0.f;
  for (int idx = blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += gridDim.x * blockDim.x) {
    const int j = idx % O, i = (idx / O) % O, c = (idx / (O * O)) % C, b = idx / (O * O * C);
    int y0, y1, x0, x1;
    float ly, lx;
    src_coord(sh, j, H, y0, y1, ly);
    src_coord(sw, i, W, x0, x1, lx);
    const float hy = 1.f - ly, hx = 1.f - lx;
    const float v00 = bilerp_fetch(in, b, c, y0, x0, C, H, W, channels_last);
    const float v01 = bilerp_fetch(in, b, c, y0, x1, C, H, W, channels_last);
    const float v10 = bilerp_fetch(in, b, c, y1, x0, C, H, W, channels_last);
    const float v11 = bilerp_fetch(in, b, c, y1, x1, C, H, W, channels_last);
    out[idx] = bilerp_blend_as_tiled(hy, hx, ly, lx, v00, v01, v10, v11);
  }
}

// ------------------------------------------------------------------------------------------------
// K2: stem conv 3x3 stride 2 pad 1 (+folded BN, ReLU6).  in: [B][C][Hin][Hin] NCHW (shared by all
// models), w: [tap][c][32], out: [K][B][Ho][Ho][32].  thread = (pixel, 4 output channels).
// ------------------------------------------------------------------------------------------------
// The layer bodies are device functions of (virtual block index, weight model k, activation slot ka): the layer-wise
// kernels call them with their blockIdx, the one-XCD-per-model persistent kernel (encoder_mega_kernel) in a loop.
__device__ __forceinline__ void stem_body(const float* __restrict__ in, const float* __restrict__ wbase,
                                          size_t model_stride, int k0, size_t w_off, size_t b_off, int B, int C, int Hin,
                                          int Ho, float* __restrict__ out, int bx, int k, int ka) {
  const float* w = wbase + (size_t)(k0 + k) * model_stride + w_off;
  const float* bias = wbase + (size_t)(k0 + k) * model_stride + b_off;
  const int total = B * Ho * Ho * 8;
  const int idx = bx * 256 + threadIdx.x;
  if (idx >= total) return;
  const int oc4 = idx & 7;
  const int pix = idx >> 3;
  const int ox = pix % Ho, oy = (pix / Ho) % Ho, b = pix / (Ho * Ho);
  float4 acc = *reinterpret_cast<const float4*>(bias + oc4 * 4);
  for (int c = 0; c < C; ++c) {
    const float* ip = in + ((size_t)b * C + c) * Hin * Hin;
    float v[9];
    float4 wv[9];
#pragma unroll
    for (int ky = 0; ky < 3; ++ky) {  // loads first (see dw_body): taps off the image count as zero
      const int iy = oy * 2 - 1 + ky;
      const int cy = min(max(iy, 0), Hin - 1);
#pragma unroll
      for (int kx = 0; kx < 3; ++kx) {
        const int ix = ox * 2 - 1 + kx;
        const int cx = min(max(ix, 0), Hin - 1);
        const bool ok = iy >= 0 && iy < Hin && ix >= 0 && ix < Hin;
        const float t = ip[(size_t)cy * Hin + cx];
        v[ky * 3 + kx] = ok ? t : 0.f;
        wv[ky * 3 + kx] = *reinterpret_cast<const float4*>(w + ((ky * 3 + kx) * C + c) * 32 + oc4 * 4);
      }
    }
#pragma unroll
    for (int t = 0; t < 9; ++t) {
      acc.x = fmaf(v[t], wv[t].x, acc.x);
      acc.y = fmaf(v[t], wv[t].y, acc.y);
      acc.z = fmaf(v[t], wv[t].z, acc.z);
      acc.w = fmaf(v[t], wv[t].w, acc.w);
    }
  }
  acc.x = relu6f(acc.x);
  acc.y = relu6f(acc.y);
  acc.z = relu6f(acc.z);
  acc.w = relu6f(acc.w);
  float* op = out + (((size_t)ka * B + b) * Ho * Ho + (size_t)oy * Ho + ox) * 32 + oc4 * 4;
  *reinterpret_cast<float4*>(op) = acc;
}

__global__ __launch_bounds__(256) void stem_kernel(const float* __restrict__ in, const float* __restrict__ wbase,
                                                    size_t model_stride, int k0, size_t w_off, size_t b_off, int B,
                                                    int C, int Hin, int Ho, float* __restrict__ out) {
  stem_body(in, wbase, model_stride, k0, w_off, b_off, B, C, Hin, Ho, out, blockIdx.x, blockIdx.z, blockIdx.z);
}

// ------------------------------------------------------------------------------------------------
// K3: depthwise 3x3 (+folded BN, ReLU6), NHWC.  w: [9][C].  thread = (output pixel, 4 channels):
// every global access is a float4 with the channel index fastest -> fully coalesced.
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ void dw_body(const float* __restrict__ in, const float* __restrict__ wbase,
                                        size_t model_stride, int k0, size_t w_off, size_t b_off, int B, int C, int Hin,
                                        int Ho, int stride, float* __restrict__ out, int bx, int k, int ka) {
  const float* w = wbase + (size_t)(k0 + k) * model_stride + w_off;
  const float* bias = wbase + (size_t)(k0 + k) * model_stride + b_off;
  const int C4 = C >> 2;
  const long total = (long)B * Ho * Ho * C4;
  const long idx = (long)bx * 256 + threadIdx.x;
  if (idx >= total) return;
  const int c4 = (int)(idx % C4);
  const long pix = idx / C4;
  const int ox = (int)(pix % Ho), oy = (int)((pix / Ho) % Ho), b = (int)(pix / ((long)Ho * Ho));
  const float* ip = in + ((size_t)ka * B + b) * Hin * Hin * C + c4 * 4;
  float4 acc = *reinterpret_cast<const float4*>(bias + c4 * 4);
  // All 18 loads are issued before the first FMA (taps off the image read a clamped address and count as zero:
  // fma(0, w, acc) == acc, so the result is the one of skipping them): one memory round trip per output instead of
  // one per tap — what a single-observation launch, or a layer of the persistent kernel, is bound by.
  float4 v[9], wv[9];
#pragma unroll
  for (int ky = 0; ky < 3; ++ky) {
    const int iy = oy * stride - 1 + ky;
    const int cy = min(max(iy, 0), Hin - 1);
#pragma unroll
    for (int kx = 0; kx < 3; ++kx) {
      const int ix = ox * stride - 1 + kx;
      const int cx = min(max(ix, 0), Hin - 1);
      const bool ok = iy >= 0 && iy < Hin && ix >= 0 && ix < Hin;
      const float4 t = *reinterpret_cast<const float4*>(ip + ((size_t)cy * Hin + cx) * C);
      v[ky * 3 + kx] = ok ? t : make_float4(0.f, 0.f, 0.f, 0.f);
      wv[ky * 3 + kx] = *reinterpret_cast<const float4*>(w + (ky * 3 + kx) * C + c4 * 4);
    }
  }
#pragma unroll
  for (int t = 0; t < 9; ++t) {
    acc.x = fmaf(v[t].x, wv[t].x, acc.x);
    acc.y = fmaf(v[t].y, wv[t].y, acc.y);
    acc.z = fmaf(v[t].z, wv[t].z, acc.z);
    acc.w = fmaf(v[t].w, wv[t].w, acc.w);
  }
  acc.x = relu6f(acc.x);
  acc.y = relu6f(acc.y);
  acc.z = relu6f(acc.z);
  acc.w = relu6f(acc.w);
  float* op = out + (((size_t)ka * B + b) * Ho * Ho + (size_t)oy * Ho + ox) * C + c4 * 4;
  *reinterpret_cast<float4*>(op) = acc;
}

__global__ __launch_bounds__(256) void dw_kernel(const float* __restrict__ in, const float* __restrict__ wbase,
                                                  size_t model_stride, int k0, size_t w_off, size_t b_off, int B,
                                                  int C, int Hin, int Ho, int stride, float* __restrict__ out) {
  dw_body(in, wbase, model_stride, k0, w_off, b_off, B, C, Hin, Ho, stride, out, blockIdx.x, blockIdx.z, blockIdx.z);
}

// ------------------------------------------------------------------------------------------------
// K4: pointwise conv as GEMM  out[M][Cout] = act(in[M][Cin] * W[Cout][Cin]^T + bias) (+ residual),
// M = B*H*W rows of one model.  Register-direct fp32-input MFMA (v_mfma_f32_16x16x4_f32: exact fp32, bitwise
// an fmaf chain): no LDS, no barriers.  The product is formed transposed, OUT^T[co][pixel]: A = 16 output
// channels of W, B = 16 pixels, both K-contiguous float4 loads (k-step (S, r) contracts channels 16S+4q+r);
// lane (n = lane & 15, q = lane >> 4) ends up with 4 consecutive output channels of pixel n -> float4 NHWC stores.
// A wave owns PT pixel tiles x CT channel tiles; with CT covering all of Cout the activations are read once.
// ------------------------------------------------------------------------------------------------
using f32x4 = __attribute__((ext_vector_type(4))) float;

// sum over each row of 16 lanes (DPP), replicated in the row
template <int CTRL>
__device__ __forceinline__ float dpp_f(float x) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), CTRL, 0xf, 0xf, true));
}
__device__ __forceinline__ float row_sum16(float x) {
  x += dpp_f<0xB1>(x);
  x += dpp_f<0x4E>(x);
  x += dpp_f<0x141>(x);
  x += dpp_f<0x140>(x);
  return x;
}

// `flags`: bit 0 = ReLU6 after the folded BN; bit 1 = global-average-pool epilogue: a 16-pixel tile is one whole
// 4x4 image (features.18), so the mean over the tile's 16 lanes is written to out[tile][Cout] instead of 16 rows.
// KSPLIT = 1: the block's 4 waves take 4 different pixel-tile groups.  KSPLIT = 4: they take the 4 quarters of the
// K range of ONE (CT x PT) tile and reduce through LDS — big register tiles (little operand re-reading from L2)
// and still enough waves when M is small (7x7 / 4x4 stages, or a single observation).
// `part`: [KSPLIT][CT * PT][64] float4 of LDS for the K-split reduction (unused with KSPLIT = 1)
// HOIST: bias and residual operands are requested before the K loop instead of in the epilogue (two fewer dependent
// memory round trips per tile; costs 4 * CT * (PT + 1) registers: the latency-bound persistent kernel only).
template <int CT, int PT, int UNROLL, int KSPLIT, bool HOIST = false, bool LF = true>
__device__ __forceinline__ void pw_body(const float* __restrict__ in, const float* __restrict__ wbase,
                                        size_t model_stride, int k0, size_t w_off, size_t b_off,
                                        const float* __restrict__ res, float* __restrict__ out, int M, int Cin, int Cout,
                                        int flags, size_t act_model_stride_in, size_t act_model_stride_out, int bx,
                                        int by, int k, int ka, float4* part) {
  // the batched tile shapes take the loads-first form (9.5 -> 9.0 ms at 512 observations), the small-launch shapes keep
  // the predicated one (see the K loop)
  constexpr bool LOADS_FIRST = LF && KSPLIT == 1;  // LF: chosen by the dispatch (launches with >= ~1024 waves)
  const int relu6 = flags & 1;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int n = lane & 15, q = lane >> 4;
  const int ptile0 = (KSPLIT == 1 ? bx * 4 + wave : bx) * PT;
  const int ctile0 = by * CT;
  if (KSPLIT == 1 && ptile0 * 16 >= M) return;
  const float* A = wbase + (size_t)(k0 + k) * model_stride + w_off;
  const float* bias = wbase + (size_t)(k0 + k) * model_stride + b_off;
  const float* X = in + (size_t)ka * act_model_stride_in;
  float* O = out + (size_t)ka * act_model_stride_out;
  const float* R = res != nullptr ? res + (size_t)ka * act_model_stride_out : nullptr;

  const float* arow[CT];
  bool aval[CT];
#pragma unroll
  for (int ct = 0; ct < CT; ++ct) {
    const int co = (ctile0 + ct) * 16 + n;
    aval[ct] = co < Cout;
    arow[ct] = A + (size_t)min(co, Cout - 1) * Cin + 4 * q;
  }
  const float* brow[PT];
#pragma unroll
  for (int pt = 0; pt < PT; ++pt) {
    const int p = (ptile0 + pt) * 16 + n;
    brow[pt] = X + (size_t)min(p, M - 1) * Cin + 4 * q;
  }
  f32x4 acc[CT][PT];
#pragma unroll
  for (int ct = 0; ct < CT; ++ct)
#pragma unroll
    for (int pt = 0; pt < PT; ++pt) acc[ct][pt] = f32x4{0.f, 0.f, 0.f, 0.f};
  float4 hb[HOIST ? CT : 1], hr[HOIST ? CT : 1][HOIST ? PT : 1];
  if (HOIST) {
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) {
      const int co = (ctile0 + ct) * 16 + 4 * q;
      hb[ct] = co < Cout ? *reinterpret_cast<const float4*>(bias + co) : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
      for (int pt = 0; pt < PT; ++pt) {
        const int p = (ptile0 + pt) * 16 + n;
        hr[ct][pt] = (R != nullptr && co < Cout && p < M) ? *reinterpret_cast<const float4*>(R + (size_t)p * Cout + co)
                                                          : make_float4(0.f, 0.f, 0.f, 0.f);
      }
    }
  }

  // UNROLL chunks per trip, all their loads issued before the first MFMA (chunks past Cin are predicated off)
  // K range of this wave (multiples of 16)
  const int kchunks = (Cin + 15) / 16;
  const int kper = (kchunks + KSPLIT - 1) / KSPLIT;
  const int kbeg = KSPLIT == 1 ? 0 : 16 * kper * wave;
  const int kend = KSPLIT == 1 ? Cin : min(Cin, 16 * kper * (wave + 1));
#pragma unroll 1
  for (int kc0 = kbeg; kc0 < kend; kc0 += 16 * UNROLL) {
#pragma unroll
   for (int u = 0; u < UNROLL; ++u) {
    const int kc = kc0 + 16 * u;
    const bool kval = kc + 4 * q < kend;  // Cin is a multiple of 8: a lane's float4 is all-valid or all-pad
    float4 av[CT], bv[PT];
    if (LOADS_FIRST) {
      // every load is unconditional (chunk 0 of the row for a lane past the K range — Cin >= 16, so in bounds — then a
      // select): a load behind a branch is waited for at the merge, which made the CT + PT loads of a chunk that many
      // memory round trips in sequence instead of one
      const int kcl = kval ? kc : 0;
#pragma unroll
      for (int ct = 0; ct < CT; ++ct) av[ct] = *reinterpret_cast<const float4*>(arow[ct] + kcl);
#pragma unroll
      for (int pt = 0; pt < PT; ++pt) bv[pt] = *reinterpret_cast<const float4*>(brow[pt] + kcl);
      // (component-wise selects: a ternary on the float4 STRUCT is lowered through a stack slot the optimiser does not
      // always remove — the operand arrays went to scratch that way)
#pragma unroll
      for (int ct = 0; ct < CT; ++ct) {
        const bool on = kval && aval[ct];
        av[ct] = make_float4(on ? av[ct].x : 0.f, on ? av[ct].y : 0.f, on ? av[ct].z : 0.f, on ? av[ct].w : 0.f);
      }
#pragma unroll
      for (int pt = 0; pt < PT; ++pt)
        bv[pt] = make_float4(kval ? bv[pt].x : 0.f, kval ? bv[pt].y : 0.f, kval ? bv[pt].z : 0.f, kval ? bv[pt].w : 0.f);
    } else {
      // small launches (one observation: 55 dependent launches at the launch floor): the predicated form is 0.16 us per
      // launch FASTER there (244 vs 254 us for the encoder; its code is half the size and these launches run cold)
#pragma unroll
      for (int ct = 0; ct < CT; ++ct)
        av[ct] = (kval && aval[ct]) ? *reinterpret_cast<const float4*>(arow[ct] + kc) : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
      for (int pt = 0; pt < PT; ++pt)
        bv[pt] = kval ? *reinterpret_cast<const float4*>(brow[pt] + kc) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) {
#pragma unroll
      for (int pt = 0; pt < PT; ++pt) {
        f32x4 c = acc[ct][pt];
        c = __builtin_amdgcn_mfma_f32_16x16x4f32(av[ct].x, bv[pt].x, c, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f32_16x16x4f32(av[ct].y, bv[pt].y, c, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f32_16x16x4f32(av[ct].z, bv[pt].z, c, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f32_16x16x4f32(av[ct].w, bv[pt].w, c, 0, 0, 0);
        acc[ct][pt] = c;
      }
    }
   }
  }
  if (KSPLIT > 1) {
    // reduce the K slices: every wave parks its partial tiles in LDS, then wave w finishes tiles t = w (mod 4)
#pragma unroll
    for (int ct = 0; ct < CT; ++ct)
#pragma unroll
      for (int pt = 0; pt < PT; ++pt)
        part[(wave * CT * PT + ct * PT + pt) * 64 + lane] =
            make_float4(acc[ct][pt][0], acc[ct][pt][1], acc[ct][pt][2], acc[ct][pt][3]);
    __syncthreads();
#pragma unroll
    for (int ct = 0; ct < CT; ++ct)
#pragma unroll
      for (int pt = 0; pt < PT; ++pt) {
        const int t = ct * PT + pt;
        if ((t & (KSPLIT - 1)) == wave) {
          float4 sum = part[t * 64 + lane];
#pragma unroll
          for (int w2 = 1; w2 < KSPLIT; ++w2) {
            const float4 o = part[(w2 * CT * PT + t) * 64 + lane];
            sum.x += o.x;
            sum.y += o.y;
            sum.z += o.z;
            sum.w += o.w;
          }
          acc[ct][pt] = f32x4{sum.x, sum.y, sum.z, sum.w};
        }
      }
  }
  // C/D layout of the 16x16 MFMA: col = lane & 15 (pixel), row = 4*(lane >> 4) + reg (channel).
  // The epilogue's operands (bias, residual) are requested here, ALL of them before any is used and none behind a
  // per-lane branch (clamped addresses): inside the store loop each was waited for on its own.
  float4 eb[CT], er[CT][PT];
#pragma unroll
  for (int ct = 0; ct < CT; ++ct) {
    const int co = (ctile0 + ct) * 16 + 4 * q;
    if (HOIST) eb[ct] = hb[ct];
    else if (LOADS_FIRST) eb[ct] = *reinterpret_cast<const float4*>(bias + (co < Cout ? co : Cout - 4));
  }
  if (!HOIST && LOADS_FIRST && R != nullptr) {  // workgroup-uniform
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) {
      const int co = (ctile0 + ct) * 16 + 4 * q;
#pragma unroll
      for (int pt = 0; pt < PT; ++pt) {
        const int p = (ptile0 + pt) * 16 + n;
        // (K-split builds: a wave finishes every KSPLIT-th tile only; the others read the first group of R, one cached line)
        const bool mine = KSPLIT == 1 || ((ct * PT + pt) & (KSPLIT - 1)) == wave;
        er[ct][pt] = *reinterpret_cast<const float4*>(R + (mine ? (size_t)(p < M ? p : M - 1) * Cout + (co < Cout ? co : Cout - 4) : (size_t)0));
      }
    }
  }
#pragma unroll
  for (int ct = 0; ct < CT; ++ct) {
    const int co = (ctile0 + ct) * 16 + 4 * q;
    if (co < Cout) {
      const float4 bb = (HOIST || LOADS_FIRST) ? eb[ct] : *reinterpret_cast<const float4*>(bias + co);
#pragma unroll
      for (int pt = 0; pt < PT; ++pt) {
        const int p = (ptile0 + pt) * 16 + n;
        if (KSPLIT != 1 && ((ct * PT + pt) & (KSPLIT - 1)) != wave) continue;  // wave-uniform
        if (flags & 2) {
          float4 v = make_float4(acc[ct][pt][0] + bb.x, acc[ct][pt][1] + bb.y, acc[ct][pt][2] + bb.z,
                                 acc[ct][pt][3] + bb.w);
          if (relu6) v = make_float4(relu6f(v.x), relu6f(v.y), relu6f(v.z), relu6f(v.w));
          if (p >= M) v = make_float4(0.f, 0.f, 0.f, 0.f);
          v.x = row_sum16(v.x) * 0.0625f;
          v.y = row_sum16(v.y) * 0.0625f;
          v.z = row_sum16(v.z) * 0.0625f;
          v.w = row_sum16(v.w) * 0.0625f;
          if (n == 0 && (ptile0 + pt) * 16 < M) *reinterpret_cast<float4*>(O + (size_t)(ptile0 + pt) * Cout + co) = v;
          continue;
        }
        if (p < M) {
          float4 v = make_float4(acc[ct][pt][0] + bb.x, acc[ct][pt][1] + bb.y, acc[ct][pt][2] + bb.z,
                                 acc[ct][pt][3] + bb.w);
          if (R != nullptr) {
            const float4 r = HOIST ? hr[ct][pt] : (LOADS_FIRST ? er[ct][pt] : *reinterpret_cast<const float4*>(R + (size_t)p * Cout + co));
            v.x += r.x;
            v.y += r.y;
            v.z += r.z;
            v.w += r.w;
          }
          if (relu6) {
            v.x = relu6f(v.x);
            v.y = relu6f(v.y);
            v.z = relu6f(v.z);
            v.w = relu6f(v.w);
          }
          *reinterpret_cast<float4*>(O + (size_t)p * Cout + co) = v;
        }
      }
    }
  }
}

template <int CT, int PT, int UNROLL, int KSPLIT, bool LF>
__global__ __launch_bounds__(256) void pw_kernel(const float* __restrict__ in, const float* __restrict__ wbase,
                                                  size_t model_stride, int k0, size_t w_off, size_t b_off,
                                                  const float* __restrict__ res, float* __restrict__ out, int M,
                                                  int Cin, int Cout, int flags, size_t act_model_stride_in,
                                                  size_t act_model_stride_out) {
  __shared__ float4 part[KSPLIT > 1 ? KSPLIT * CT * PT * 64 : 1];
  pw_body<CT, PT, UNROLL, KSPLIT, false, LF>(in, wbase, model_stride, k0, w_off, b_off, res, out, M, Cin, Cout, flags,
                                             act_model_stride_in, act_model_stride_out, blockIdx.x, blockIdx.y,
                                             blockIdx.z, blockIdx.z, part);
}

template <int CT, int PT, int UNROLL, int KSPLIT, bool LF = (KSPLIT == 1)>
void launch_pw(const float* in, const float* enc_w, size_t ms, int k0, int kc, const Layer& l, const float* res,
               float* dst, int M, bool pool, hipStream_t s) {
  const int n_pt = (M + 15) / 16, n_ct = (l.cout + 15) / 16;
  const int groups = (n_pt + PT - 1) / PT;
  const dim3 grid(KSPLIT == 1 ? (groups + 3) / 4 : groups, (n_ct + CT - 1) / CT, kc);
  hipLaunchKernelGGL((pw_kernel<CT, PT, UNROLL, KSPLIT, LF>), grid, dim3(256), 0, s, in, enc_w, ms, k0, l.w_off, l.b_off,
                     res, dst, M, l.cin, l.cout, l.relu6 | (pool ? 2 : 0), (size_t)M * l.cin,
                     pool ? (size_t)(M / 16) * l.cout : (size_t)M * l.cout);
}

// Tile choice: the biggest wave tile that still yields >= ~1024 waves.  When even that is impossible with one
// wave per tile (small M) and the reduction is long enough, the 4 waves of a block split K instead.
void dispatch_pw(const float* in, const float* enc_w, size_t ms, int k0, int kc, const Layer& l, const float* res,
                 float* dst, int M, bool pool, hipStream_t s) {
  const long n_pt = (M + 15) / 16, n_ct = (l.cout + 15) / 16;
  auto jobs = [&](int ct, int pt) { return ((n_pt + pt - 1) / pt) * ((n_ct + ct - 1) / ct) * kc; };
  const long want = 1024;
#define PW_GO(CT_, PT_, U_, KS_) return launch_pw<CT_, PT_, U_, KS_>(in, enc_w, ms, k0, kc, l, res, dst, M, pool, s)
  if (n_ct >= 5 && jobs(6, 2) >= want) PW_GO(6, 2, 2, 1);
  if (n_ct >= 3 && jobs(4, 2) >= want) PW_GO(4, 2, 2, 1);
  if (n_ct >= 2 && jobs(2, 2) >= want) PW_GO(2, 2, 4, 1);
  if (l.cin >= 128) {  // >= 8 K chunks: split K over the block's waves
    if (n_ct >= 5 && jobs(6, 2) * 4 >= want) PW_GO(6, 2, 2, 4);
    if (n_ct >= 3 && jobs(4, 2) * 4 >= want) PW_GO(4, 2, 2, 4);
    if (n_ct >= 2 && jobs(2, 2) * 4 >= want) PW_GO(2, 2, 4, 4);
    if (jobs(1, 2) * 4 >= want) PW_GO(1, 2, 4, 4);
    PW_GO(1, 1, 4, 4);
  }
  if (jobs(1, 2) >= want) PW_GO(1, 2, 8, 1);
  if (jobs(1, 1) >= want) PW_GO(1, 1, 8, 1);
  return launch_pw<1, 1, 8, 1, false>(in, enc_w, ms, k0, kc, l, res, dst, M, pool, s);  // small launch: predicated loads
#undef PW_GO
}

// ------------------------------------------------------------------------------------------------
// K5: global average pool -> classifier Linear(1280,128).  One block per (observation, model, group of
// 16 outputs): the pooled vector is rebuilt per block (the 16x1280 activation tile is L2-resident),
// each wave owns 4 outputs and strides the 1280 inputs with coalesced row reads.
// ------------------------------------------------------------------------------------------------
constexpr int CLS_GROUP = 16;

__device__ __forceinline__ void cls_body(const float* __restrict__ act, const float* __restrict__ wbase,
                                         size_t model_stride, int k0, size_t cls_w, size_t cls_b, int B, int HW,
                                         float* __restrict__ feat, int b, int k, int ka, int og, float* pooled) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float* W = wbase + (size_t)(k0 + k) * model_stride;
  const float* a = act + ((size_t)ka * B + b) * HW * LAST_C;
  const float inv = 1.0f / (float)HW;
  for (int c = tid; c < LAST_C; c += 256) {
    float s = 0.f;
    for (int p = 0; p < HW; ++p) s += a[(size_t)p * LAST_C + c];
    pooled[c] = s * inv;
  }
  __syncthreads();
#pragma unroll
  for (int q = 0; q < CLS_GROUP / 4; ++q) {
    const int o = og * CLS_GROUP + wave * (CLS_GROUP / 4) + q;
    const float* wr = W + cls_w + (size_t)o * LAST_C;
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < LAST_C / 64; ++i) s = fmaf(wr[i * 64 + lane], pooled[i * 64 + lane], s);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) s += __shfl_xor(s, d, 64);
    if (lane == 0) feat[((size_t)ka * B + b) * FEAT + o] = s + W[cls_b + o];
  }
}

__global__ __launch_bounds__(256) void cls_kernel(const float* __restrict__ act, const float* __restrict__ wbase,
                                                   size_t model_stride, int k0, size_t cls_w, size_t cls_b, int B,
                                                   int HW, float* __restrict__ feat) {
  __shared__ float pooled[LAST_C];
  cls_body(act, wbase, model_stride, k0, cls_w, cls_b, B, HW, feat, blockIdx.x, blockIdx.y, blockIdx.y, blockIdx.z,
           pooled);
}

// classifier on the matrix cores for already pooled features (HW == 1: the bf16 encoder's features.18 epilogue pools):
// one workgroup = 16 observations x 16 outputs on v_mfma_f32_16x16x4_f32, both operands read as 16-byte groups along K
// (lane (n, q) holds k = 16 j + 4 q + e of row n: MFMA e of group j contracts the four k with that e — a partition of
// K, so the order of the instruction's internal k does not matter).  fp32 in, fp32 accumulate; the summation order
// differs from cls_kernel's lane-strided chain (last-bit differences).  62 -> 26 us at 512 observations x 4 models
// (a 16 x 64 merger on the same instruction, one wave per 16 observations, was 19 us against merger_kernel's 17).
__global__ __launch_bounds__(256) void cls_mfma_kernel(const float* __restrict__ pooled, const float* __restrict__ wbase,
                                                        size_t model_stride, int k0, size_t cls_w, size_t cls_b, int B,
                                                        float* __restrict__ feat) {
  using f32x4 = __attribute__((ext_vector_type(4))) float;
  __shared__ f32x4 part[3][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int n = lane & 15, q = lane >> 4;
  const int k = blockIdx.y;
  const int bt = blockIdx.x;              // 16-observation tile
  const int ot = blockIdx.z;              // 16-output tile
  const float* W = wbase + (size_t)(k0 + k) * model_stride;
  const int b = min(bt * 16 + n, B - 1);  // rows past B are computed on a valid row and not stored
  // the four waves of the workgroup split K (round 5: one wave walked all of it, 80 dependent load -> MFMA rounds;
  // 26 -> 21 us at 512 observations x 4 models); their partial tiles are summed in wave order through LDS
  constexpr int JW = LAST_C / 16 / 4;
  const float4* xr = reinterpret_cast<const float4*>(pooled + ((size_t)k * B + b) * LAST_C) + q + 4 * JW * wave;
  const float4* wr = reinterpret_cast<const float4*>(W + cls_w + (size_t)(ot * 16 + n) * LAST_C) + q + 4 * JW * wave;
  f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = acc0;
#pragma unroll 5
  for (int j = 0; j < JW; ++j) {
    const float4 a = wr[4 * j], x = xr[4 * j];
    acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, x.x, acc0, 0, 0, 0);
    acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, x.y, acc1, 0, 0, 0);
    acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, x.z, acc0, 0, 0, 0);
    acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, x.w, acc1, 0, 0, 0);
  }
  f32x4 sum = acc0 + acc1;
  if (wave > 0) part[wave - 1][lane] = sum;
  __syncthreads();
  if (wave > 0) return;
  sum = ((sum + part[0][lane]) + part[1][lane]) + part[2][lane];
  // lane (n = observation, q): outputs 4 q + r
  const int bo = bt * 16 + n;
  if (bo < B) {
    const float4 bias = *reinterpret_cast<const float4*>(W + cls_b + ot * 16 + 4 * q);
    float4 o;
    o.x = sum[0] + bias.x;
    o.y = sum[1] + bias.y;
    o.z = sum[2] + bias.z;
    o.w = sum[3] + bias.w;
    *reinterpret_cast<float4*>(feat + ((size_t)k * B + bo) * FEAT + ot * 16 + 4 * q) = o;
  }
}

// ------------------------------------------------------------------------------------------------
// K6: cat(feat128, vec5) -> merger 3x(Linear+ReLU) (dim/model.py:206-217).  One wave per (obs, model):
// lane j owns output unit j, inputs broadcast from LDS.
// ------------------------------------------------------------------------------------------------
// Threads 0..63 of the block work; every thread of the block reaches the barriers.  v: [FEAT + VEC + 3], hbuf: [2][HID].
__device__ __forceinline__ void merger_body(const float* __restrict__ feat, const float* __restrict__ wbase,
                                            size_t model_stride, int k0, size_t m0w, size_t m0b, size_t m1w, size_t m1b,
                                            size_t m2w, size_t m2b, const float* __restrict__ vec, int B,
                                            float* __restrict__ z, int b, int k, int kf, int kz, float* v, float* hbuf) {
  const int tid = threadIdx.x;
  const bool on = tid < 64;
  const float* W = wbase + (size_t)(k0 + k) * model_stride;
  if (on) {
    for (int i = tid; i < FEAT; i += 64) v[i] = feat[((size_t)kf * B + b) * FEAT + i];
    if (tid < VEC) v[FEAT + tid] = vec[(size_t)b * VEC + tid];
  }
  __syncthreads();
  if (on) {
    const float* wr = W + m0w + (size_t)tid * (FEAT + VEC);
    float s = W[m0b + tid];
    for (int i = 0; i < FEAT + VEC; ++i) s = fmaf(wr[i], v[i], s);
    hbuf[tid] = fmaxf(s, 0.f);
  }
  __syncthreads();
  if (on) {
    const float* wr = W + m1w + (size_t)tid * HID;
    float s = W[m1b + tid];
    for (int i = 0; i < HID; ++i) s = fmaf(wr[i], hbuf[i], s);
    hbuf[HID + tid] = fmaxf(s, 0.f);
  }
  __syncthreads();
  if (on) {
    const float* wr = W + m2w + (size_t)tid * HID;
    float s = W[m2b + tid];
    for (int i = 0; i < HID; ++i) s = fmaf(wr[i], hbuf[HID + i], s);
    z[((size_t)kz * B + b) * HID + tid] = fmaxf(s, 0.f);
  }
}

__global__ __launch_bounds__(64) void merger_kernel(const float* __restrict__ feat, const float* __restrict__ wbase,
                                                     size_t model_stride, int k0, size_t m0w, size_t m0b, size_t m1w,
                                                     size_t m1b, size_t m2w, size_t m2b,
                                                     const float* __restrict__ vec, int B, float* __restrict__ z) {
  __shared__ float v[FEAT + VEC + 3];
  __shared__ float hbuf[2 * HID];
  merger_body(feat, wbase, model_stride, k0, m0w, m0b, m1w, m1b, m2w, m2b, vec, B, z, blockIdx.x, blockIdx.y,
              blockIdx.y, blockIdx.y, v, hbuf);
}

// ------------------------------------------------------------------------------------------------
// One launch for the whole encoder of a SMALL batch (online: one observation per call).  Layer by layer the B = 1
// encoder is 55 dependent launches of ~1 us of work each, and a dependent launch costs ~4.8 us inside a hipGraph
// (profiles/r3/online_trace_v1.txt): 283 us.  A persistent kernel has to replace the launch boundary by a barrier
// among its workgroups, and a device-wide barrier is no cheaper (tools/micro/grid_barrier.hip: 17-27 us for 256
// workgroups — every arrival is a round trip to the memory side).  But the K ensemble members are independent until
// the plan search, the hardware places workgroup i of a launch on XCD i % 8 (tools/micro/xcd_barrier.hip), and the
// workgroups of ONE XCD share an L2: model k runs on XCD k % 8 only, its activations never leave that L2, and the
// barrier between two layers is an atomic counter that lives in that L2 — ~1 us per layer for 32 workgroups
// (xcd_barrier.hip mode 1), no cache maintenance:
//   * arrival: s_waitcnt vmcnt(0) (the TCP is write-through: the workgroup's stores are in the L2 then), one atomic add;
//     wait: returning atomics (performed in the L2, never served by a TCP);
//   * every layer writes its own region of the per-model arena, so no cache line that some TCP may hold is ever
//     rewritten inside the launch (a TCP is invalidated at the launch boundary): the consumers' loads miss to the L2.
// A workgroup that finds itself on another XCD than blockIdx % 8, or a barrier that waits longer than 20 ms, raises
// the status word (pinned host memory) and the launch drains: the caller falls back to the layer-wise launches.
// ------------------------------------------------------------------------------------------------
constexpr unsigned MEGA_NONE = 0xffffffffu;
constexpr int MEGA_MAX_LAYERS = 56;
struct MegaLayer {
  uint32_t w_off, b_off;    // floats into the model's blob
  uint32_t src, dst, res;   // floats into the model's arena (src NONE: the network input; res NONE: no residual)
  uint32_t M;               // pointwise: rows = B * h_out^2
  uint16_t cin, cout, gx, gy;  // virtual grid of the layer body
  uint8_t kind, variant, h_in, h_out, stride, flags, pad0, pad1;
};
struct MegaArgs {
  const float* visual;
  const float* vec;
  const float* wbase;
  float* arena;
  float* z;
  float* feat;             // nullable: classifier output for the caller
  unsigned* sync;          // [8][2][32]: per XCD a barrier counter and an exit counter, one 128-byte line each
  int* status;             // pinned host word
  unsigned long long* ticks;  // nullable (development): wall clock after every layer of model 0
  size_t model_stride, arena_model_stride;
  size_t cls_w, cls_b, m0w, m0b, m1w, m1b, m2w, m2b;
  uint32_t last_off, feat_off;
  int k0, kc, B, C, last_hw, n_layers;
  MegaLayer layers[MEGA_MAX_LAYERS];
};
static_assert(sizeof(MegaArgs) <= 4096, "kernel arguments are limited to 4 KB");

__device__ __forceinline__ unsigned xcc_id() { return __builtin_amdgcn_s_getreg(63508) & 0xf; }  // HW_REG_XCC_ID

__device__ __forceinline__ bool xcd_barrier(unsigned* ctr, unsigned target, int* s_flag) {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0) {
    __hip_atomic_fetch_add(ctr, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const long long t0 = wall_clock64();
    int ok = 1;
    while (__hip_atomic_fetch_add(ctr, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < target) {
      if (wall_clock64() - t0 > 2000000) {  // 20 ms of the 100 MHz wall clock
        ok = 0;
        break;
      }
    }
    *s_flag = ok;
  }
  __syncthreads();
  return *s_flag != 0;
}

template <int CT, int PT, int UNROLL, int KSPLIT>
__device__ __forceinline__ void mega_pw(const MegaArgs& a, const MegaLayer& L, const float* src, const float* res,
                                        float* dst, int k, int rank, int P, float4* part) {
  const int nvb = (int)L.gx * L.gy;
#pragma unroll 1
  for (int vb = rank; vb < nvb; vb += P) {
    const int by = vb / L.gx, bx = vb - by * L.gx;
    pw_body<CT, PT, UNROLL, KSPLIT, true>(src, a.wbase, a.model_stride, a.k0, L.w_off, L.b_off, res, dst, (int)L.M,
                                          L.cin, L.cout, L.flags, 0, 0, bx, by, k, 0, part);
    if (KSPLIT > 1) __syncthreads();  // `part` is reused by the next virtual block
  }
}

constexpr int MEGA_PART_F4 = 4 * 8 * 64;  // K-split scratch of the largest pointwise variant (CT * PT = 8)

__global__ __launch_bounds__(256) void encoder_mega_kernel(const MegaArgs a) {
  __shared__ float4 part[MEGA_PART_F4];
  __shared__ int s_flag;
  const int P = gridDim.x >> 3, rank = blockIdx.x >> 3;
  const unsigned x = xcc_id();
  if (x != (blockIdx.x & 7u)) {  // not where the barrier protocol assumes this workgroup to be
    if (threadIdx.x == 0) __hip_atomic_store(a.status, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    return;  // the workgroups that wait for this one time out and drain
  }
  if ((int)x >= a.kc) return;
  unsigned* ctr = a.sync + x * 64;
  unsigned* done = ctr + 32;
  unsigned epoch = 0;
  const int B = a.B;
#pragma unroll 1
  for (int kr = (int)x; kr < a.kc; kr += 8) {
    float* arena = a.arena + (size_t)kr * a.arena_model_stride;
#pragma unroll 1
    for (int li = 0; li < a.n_layers; ++li) {
      const MegaLayer& L = a.layers[li];
      // Warm the L2 with the NEXT layer's weights (one dword per 128-byte line, spread over the XCD's workgroups):
      // they arrive from HBM / the memory-side cache while this layer computes, instead of after its barrier.
      {
        const bool last = li + 1 == a.n_layers;
        const size_t w0 = last ? a.cls_w : a.layers[li + 1].w_off;
        const size_t w1 = last ? a.m2b + HID : (size_t)a.layers[li + 1].b_off + a.layers[li + 1].cout;
        const float* wp = a.wbase + (size_t)(a.k0 + kr) * a.model_stride;
        for (size_t i = w0 + ((size_t)rank * 256 + threadIdx.x) * 32; i < w1; i += (size_t)P * 256 * 32) {
          float sink;
          asm volatile("global_load_dword %0, %1, off" : "=v"(sink) : "v"(wp + i) : "memory");
        }
      }
      const float* src = L.src == MEGA_NONE ? a.visual : arena + L.src;
      const float* res = L.res == MEGA_NONE ? nullptr : arena + L.res;
      float* dst = arena + L.dst;
      if (L.kind == L_STEM) {
#pragma unroll 1
        for (int vb = rank; vb < (int)L.gx; vb += P)
          stem_body(src, a.wbase, a.model_stride, a.k0, L.w_off, L.b_off, B, a.C, L.h_in, L.h_out, dst, vb, kr, 0);
      } else if (L.kind == L_DW) {
#pragma unroll 1
        for (int vb = rank; vb < (int)L.gx; vb += P)
          dw_body(src, a.wbase, a.model_stride, a.k0, L.w_off, L.b_off, B, L.cout, L.h_in, L.h_out, L.stride, dst, vb, kr,
                  0);
      } else {
        switch (L.variant) {
          case 0: mega_pw<1, 1, 8, 1>(a, L, src, res, dst, kr, rank, P, part); break;
          case 1: mega_pw<1, 2, 8, 1>(a, L, src, res, dst, kr, rank, P, part); break;
          case 2: mega_pw<2, 2, 4, 1>(a, L, src, res, dst, kr, rank, P, part); break;
          case 3: mega_pw<4, 2, 2, 1>(a, L, src, res, dst, kr, rank, P, part); break;
          case 4: mega_pw<1, 1, 8, 4>(a, L, src, res, dst, kr, rank, P, part); break;
          case 5: mega_pw<1, 2, 8, 4>(a, L, src, res, dst, kr, rank, P, part); break;
          case 6: mega_pw<2, 2, 4, 4>(a, L, src, res, dst, kr, rank, P, part); break;
          default: mega_pw<4, 2, 2, 4>(a, L, src, res, dst, kr, rank, P, part); break;
        }
      }
      ++epoch;
      if (a.ticks != nullptr && kr == 0 && rank == 0 && threadIdx.x == 0) a.ticks[64 + li] = wall_clock64();
      if (!xcd_barrier(ctr, epoch * (unsigned)P, &s_flag)) {
        if (threadIdx.x == 0) __hip_atomic_store(a.status, 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        return;
      }
      if (a.ticks != nullptr && kr == 0 && rank == 0 && threadIdx.x == 0) a.ticks[li] = wall_clock64();
    }
    // pool (if features.18 did not) + classifier, then the merger
    float* feat = a.feat != nullptr ? a.feat + (size_t)kr * B * FEAT : arena + a.feat_off;
    float* scratch = reinterpret_cast<float*>(part);
#pragma unroll 1
    for (int vb = rank; vb < B * (FEAT / CLS_GROUP); vb += P) {
      const int b = vb / (FEAT / CLS_GROUP), og = vb - b * (FEAT / CLS_GROUP);
      cls_body(arena + a.last_off, a.wbase, a.model_stride, a.k0, a.cls_w, a.cls_b, B, a.last_hw, feat, b, kr, 0, og,
               scratch);
      __syncthreads();
    }
    ++epoch;
    if (!xcd_barrier(ctr, epoch * (unsigned)P, &s_flag)) {
      if (threadIdx.x == 0) __hip_atomic_store(a.status, 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      return;
    }
#pragma unroll 1
    for (int b = rank; b < B; b += P) {
      merger_body(feat, a.wbase, a.model_stride, a.k0, a.m0w, a.m0b, a.m1w, a.m1b, a.m2w, a.m2b, a.vec, B,
                  a.z + (size_t)kr * B * HID, b, kr, 0, 0, scratch, scratch + 256);
      __syncthreads();
    }
    if (a.ticks != nullptr && kr == 0 && rank == 0 && threadIdx.x == 0) a.ticks[a.n_layers] = wall_clock64();
  }
  // the last workgroup of this XCD to leave re-arms the counters for the next launch (every workgroup that leaves
  // has passed the final barrier, so nobody still reads them)
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned old = __hip_atomic_fetch_add(done, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (old == (unsigned)P - 1u) {
      __hip_atomic_store(ctr, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(done, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

__global__ void mega_probe_kernel(int* xcc) {
  if (threadIdx.x == 0) xcc[blockIdx.x] = (int)xcc_id();
}

}  // namespace

// ------------------------------------------------------------------------------------------------
// host: plan, BN folding, launch sequence
// ------------------------------------------------------------------------------------------------
EncoderPlan build_encoder_plan(int in_channels) {
  EncoderPlan p;
  p.in_channels = in_channels;
  size_t off = 0;
  size_t max_act = 0;
  auto add = [&](int kind, int cin, int cout, int h_in, int stride, int relu6, int residual, int src, int dst,
                 int res) {
    Layer l;
    l.kind = kind;
    l.cin = cin;
    l.cout = cout;
    l.h_in = h_in;
    l.stride = stride;
    l.h_out = kind == L_PW ? h_in : conv_out(h_in, stride);
    l.relu6 = relu6;
    l.residual = residual;
    l.src = src;
    l.dst = dst;
    l.res = res;
    const size_t wn = kind == L_STEM ? (size_t)9 * cin * cout : (kind == L_DW ? (size_t)9 * cout : (size_t)cin * cout);
    l.w_off = off;
    off += (wn + 3) / 4 * 4;
    l.b_off = off;
    off += ((size_t)cout + 3) / 4 * 4;
    const size_t act = (size_t)l.h_out * l.h_out * cout;
    if (act > max_act) max_act = act;
    p.layers.push_back(l);
    return l.h_out;
  };
  int h = add(L_STEM, in_channels, STEM_C, IN_HW, 2, 1, 0, -1, 0, -1);
  int cur = 0, inp = STEM_C;
  for (int s = 0; s < 7; ++s) {
    const int t = IR_SETTING[s][0], c = IR_SETTING[s][1], n = IR_SETTING[s][2], st = IR_SETTING[s][3];
    for (int i = 0; i < n; ++i) {
      const int stride = i == 0 ? st : 1;
      const int hidden = inp * t;
      const int e = (cur + 1) & 3, d = (cur + 2) & 3, o = (cur + 3) & 3;
      int src = cur;
      FusedBlock fb;
      fb.expand = -1;
      fb.src = cur;
      fb.dst = o;
      if (t != 1) {
        fb.expand = (int)p.layers.size();
        add(L_PW, inp, hidden, h, 1, 1, 0, cur, e, -1);
        src = e;
      }
      fb.dw = (int)p.layers.size();
      const int h2 = add(L_DW, hidden, hidden, h, stride, 1, 0, src, d, -1);
      const int residual = (stride == 1 && inp == c) ? 1 : 0;
      fb.project = (int)p.layers.size();
      add(L_PW, hidden, c, h2, 1, 0, residual, d, o, residual ? cur : -1);
      p.blocks.push_back(fb);
      cur = o;
      inp = c;
      h = h2;
    }
  }
  const int last = (cur + 1) & 3;
  add(L_PW, inp, LAST_C, h, 1, 1, 0, cur, last, -1);
  p.final_buf = last;
  p.final_hw = h;
  auto lin = [&](size_t n) {
    const size_t o = off;
    off += (n + 3) / 4 * 4;
    return o;
  };
  p.cls_w_off = lin((size_t)FEAT * LAST_C);
  p.cls_b_off = lin(FEAT);
  const int sizes[4] = {FEAT + VEC, HID, HID, HID};
  for (int i = 0; i < 3; ++i) {
    p.mrg_w_off[i] = lin((size_t)sizes[i + 1] * sizes[i]);
    p.mrg_b_off[i] = lin(sizes[i + 1]);
  }
  p.blob_floats = off;
  p.max_act_floats = max_act;
  p.split_rows = split_rows_layout(p);
  p.split_tiles = split_tile_layout(p);
  return p;
}

bool fold_and_pack(const EncoderPlan& plan, const float* packed, size_t numel, std::vector<float>& enc,
                   std::vector<float>& flow, std::vector<float>& mw, std::vector<uint32_t>& mh, const char** err,
                   float* split_wmax) {
  enc.assign(plan.blob_floats, 0.f);
  flow.assign(FW_SIZE, 0.f);
  size_t pos = 0;
  auto need = [&](size_t n) { return pos + n <= numel; };
  for (const Layer& l : plan.layers) {
    const size_t per_out = l.kind == L_STEM ? (size_t)l.cin * 9 : (l.kind == L_DW ? 9 : (size_t)l.cin);
    const size_t wn = per_out * l.cout;
    if (!need(wn + 4 * (size_t)l.cout)) {
      *err = "packed state_dict too short (encoder)";
      return false;
    }
    const float* w = packed + pos;
    const float* gamma = w + wn;
    const float* beta = gamma + l.cout;
    const float* mean = beta + l.cout;
    const float* var = mean + l.cout;
    pos += wn + 4 * (size_t)l.cout;
    for (int oc = 0; oc < l.cout; ++oc) {
      const double scale = (double)gamma[oc] / std::sqrt((double)var[oc] + BN_EPS);
      enc[l.b_off + oc] = (float)((double)beta[oc] - (double)mean[oc] * scale);
      for (size_t i = 0; i < per_out; ++i) {
        const float v = (float)((double)w[(size_t)oc * per_out + i] * scale);
        if (l.kind == L_STEM) {
          // reference [oc][c][ky][kx] -> [tap][c][oc]
          const int c = (int)(i / 9), tap = (int)(i % 9);
          enc[l.w_off + ((size_t)tap * l.cin + c) * l.cout + oc] = v;
        } else if (l.kind == L_DW) {
          enc[l.w_off + i * l.cout + oc] = v;  // [oc][1][ky][kx] -> [tap][oc]
        } else {
          enc[l.w_off + (size_t)oc * l.cin + i] = v;  // [oc][cin] kept
        }
      }
    }
  }
  auto copy = [&](size_t dst_off, size_t n) {
    if (!need(n)) return false;
    std::memcpy(enc.data() + dst_off, packed + pos, n * sizeof(float));
    pos += n;
    return true;
  };
  bool ok = copy(plan.cls_w_off, (size_t)FEAT * LAST_C) && copy(plan.cls_b_off, FEAT);
  const int sizes[4] = {FEAT + VEC, HID, HID, HID};
  for (int i = 0; i < 3 && ok; ++i)
    ok = copy(plan.mrg_w_off[i], (size_t)sizes[i + 1] * sizes[i]) && copy(plan.mrg_b_off[i], sizes[i + 1]);
  if (!ok) {
    *err = "packed state_dict too short (classifier/merger)";
    return false;
  }
  // ---- flow: GRUCell + head, re-laid lane-major (flow.h) ----
  const size_t fl = 192 * 2 + 192 * 64 + 192 + 192 + 32 * 64 + 32 + 4 * 32 + 4;
  if (pos + fl != numel) {
    *err = "packed state_dict has the wrong length";
    return false;
  }
  const float* wih = packed + pos;
  const float* whh = wih + 192 * 2;
  const float* bih = whh + 192 * 64;
  const float* bhh = bih + 192;
  const float* w1 = bhh + 192;
  const float* b1 = w1 + 32 * 64;
  const float* w2 = b1 + 32;
  const float* b2 = w2 + 4 * 32;
  for (int g = 0; g < 3; ++g)
    for (int i4 = 0; i4 < 16; ++i4)
      for (int j = 0; j < 64; ++j)
        for (int q = 0; q < 4; ++q)
          flow[FW_WHH + (((size_t)(g * 16 + i4) * 64 + j) * 4) + q] = whh[(size_t)(g * 64 + j) * 64 + 4 * i4 + q];
  for (int g = 0; g < 3; ++g)
    for (int j = 0; j < 64; ++j) {
      flow[FW_WIH + (g * 2 + 0) * 64 + j] = wih[(g * 64 + j) * 2 + 0];
      flow[FW_WIH + (g * 2 + 1) * 64 + j] = wih[(g * 64 + j) * 2 + 1];
      flow[FW_BIH + g * 64 + j] = bih[g * 64 + j];
      flow[FW_BHH + g * 64 + j] = bhh[g * 64 + j];
    }
  for (int j = 0; j < 64; ++j) {
    flow[FW_B1 + j] = b1[j & 31];
    flow[FW_W2 + j] = w2[(2 * (j >> 5) + 0) * 32 + (j & 31)];
    flow[FW_W2 + 64 + j] = w2[(2 * (j >> 5) + 1) * 32 + (j & 31)];
  }
  for (int c = 0; c < 4; ++c) flow[FW_B2 + c] = b2[c];
  std::memcpy(flow.data() + FW_W1, w1, 32 * 64 * sizeof(float));

  // ---- operands of the MFMA search kernel (flow_phase.hip; the layout is round 1's): lane (m = lane & 15, q = lane >> 4) ----
  mw.assign(MW_SIZE, 0.f);
  auto F = [&](int idx, int lane) -> float& { return mw[(size_t)(idx / 4) * 256 + lane * 4 + (idx & 3)]; };
  auto Bk = [&](int f4, int lane, int comp) -> float& { return mw[MWF_FLOATS + ((size_t)f4 * 64 + lane) * 4 + comp]; };
  for (int lane = 0; lane < 64; ++lane) {
    const int m = lane & 15, q = lane >> 4;
    for (int g = 0; g < 3; ++g)
      for (int up = 0; up < 4; ++up)
        for (int u = 0; u < 4; ++u)
          for (int r = 0; r < 4; ++r)
            F((g * 4 + up) * 16 + u * 4 + r, lane) = whh[(size_t)(g * 64 + 16 * up + m) * 64 + 16 * u + 4 * q + r];
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
        F(192 + a * 4 + up, lane) = v;
      }
    }
    for (int mt = 0; mt < 2; ++mt) {
      for (int u = 0; u < 4; ++u)
        for (int r = 0; r < 4; ++r) F(208 + mt * 16 + u * 4 + r, lane) = w1[(16 * mt + m) * 64 + 16 * u + 4 * q + r];
      F(240 + mt, lane) = q == 2 ? b1[16 * mt + m] : 0.f;
      for (int r = 0; r < 4; ++r) F(242 + mt * 4 + r, lane) = w2[(m & 3) * 32 + 16 * mt + 4 * q + r];
    }
    F(250, lane) = q == 2 ? b2[m & 3] : 0.f;
    // adjoint operands
    Bk(0, lane, 0) = w2[q * 32 + m];
    Bk(0, lane, 1) = w2[q * 32 + 16 + m];
    for (int mt = 0; mt < 2; ++mt)
      for (int r = 0; r < 4; ++r)
        for (int ut = 0; ut < 4; ++ut) Bk(1 + mt * 4 + r, lane, ut) = w1[(16 * mt + 4 * q + r) * 64 + 16 * ut + m];
    for (int g = 0; g < 3; ++g)
      for (int up = 0; up < 4; ++up)
        for (int r = 0; r < 4; ++r) {
          const int s = (g * 4 + up) * 4 + r;
          const int j = g * 64 + 16 * up + 4 * q + r;
          for (int ut = 0; ut < 4; ++ut) Bk(9 + s, lane, ut) = whh[(size_t)j * 64 + 16 * ut + m];
          Bk(57 + s / 4, lane, s & 3) = wih[j * 2 + (m & 1)];
        }
  }
  // ---- operands of the split-f16 search kernel (flow_split.hip) ----
  const float wmax = pack_split_operands(mw.data(), wih, whh, w1, bih, bhh, b1, w2, b2, mh);
  if (split_wmax != nullptr) *split_wmax = wmax;
  return true;
}

hipError_t launch_transform(const float* in, int B, int C, int H, int W, int channels_last, int out_hw, float* out,
                            hipStream_t s) {
  const float scale = out_hw > 1 ? (float)((H > W ? H : W) - 1) / (float)(out_hw - 1) : 0.f;
  const bool tiled = scale * (TR_T - 1) + 3.f <= (float)TR_P && C >= 1 && C <= 3;
  if (tiled && channels_last) {
    if (C == 1) launch_transform_tiled<1, true>(in, nullptr, B, H, W, out_hw, out, s);
    if (C == 2) launch_transform_tiled<2, true>(in, nullptr, B, H, W, out_hw, out, s);
    if (C == 3) launch_transform_tiled<3, true>(in, nullptr, B, H, W, out_hw, out, s);
  } else if (tiled) {
    if (C == 1) launch_transform_tiled<1, false>(in, nullptr, B, H, W, out_hw, out, s);
    if (C == 2) launch_transform_tiled<2, false>(in, nullptr, B, H, W, out_hw, out, s);
    if (C == 3) launch_transform_tiled<3, false>(in, nullptr, B, H, W, out_hw, out, s);
  } else {
    const int total = B * C * out_hw * out_hw;
    int grid = (total + 255) / 256;
    if (grid > 4096) grid = 4096;
    hipLaunchKernelGGL(transform_generic_kernel, dim3(grid), dim3(256), 0, s, in, B, C, H, W, channels_last, out_hw, out);
  }
  return hipGetLastError();
}

// coded BEV (uint8 indices into a 256-entry float table), channels-last, the tiled kernel's shapes only
bool transform_coded_supported(int C, int H, int W, int out_hw) {
  const float scale = out_hw > 1 ? (float)((H > W ? H : W) - 1) / (float)(out_hw - 1) : 0.f;
  return scale * (TR_T - 1) + 3.f <= (float)TR_P && C >= 1 && C <= 3;
}
hipError_t launch_transform_coded(const uint8_t* in, const float* lut, int B, int C, int H, int W, int out_hw, float* out,
                                  hipStream_t s) {
  if (C == 1) launch_transform_tiled<1, true, uint8_t>(in, lut, B, H, W, out_hw, out, s);
  if (C == 2) launch_transform_tiled<2, true, uint8_t>(in, lut, B, H, W, out_hw, out, s);
  if (C == 3) launch_transform_tiled<3, true, uint8_t>(in, lut, B, H, W, out_hw, out, s);
  return hipGetLastError();
}

template <int C>
static hipError_t launch_gather_batch_c(const uint8_t* codes, const float* lut, const int64_t* rows, int B, int64_t n, int H,
                                        int W, int O, const float* vec, const float* future, int L, int T, int stride,
                                        const float* mode, float* visual, float* vec_out, float* target, float* mode_out,
                                        hipStream_t s) {
  constexpr int ROW = TR_P * C;
  const size_t lds = ((size_t)(ROW + 1) * TR_P + 256) * sizeof(float);  // C = 4: 74.3 KB patch + 1 KB table
  if (lds > 64 * 1024) {  // per device: above 64 KB the dynamic LDS size needs the opt-in (160 KB per CU on gfx950)
    static bool attr_set[64] = {};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return hipGetLastError();
    if (dev >= 0 && dev < 64 && !attr_set[dev]) {
      hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(gather_batch_kernel<C>),
                                         hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
      if (e != hipSuccess) return e;
      attr_set[dev] = true;
    }
  }
  const int tiles = (O + TR_T - 1) / TR_T;
  hipLaunchKernelGGL((gather_batch_kernel<C>), dim3(tiles, tiles, B), dim3(256), lds, s, codes, lut, rows, n, H, W, O, vec,
                     future, L, T, stride, mode, visual, vec_out, target, mode_out);
  return hipGetLastError();
}

bool gather_batch_supported(int C, int H, int W, int out_hw) {
  const float scale = out_hw > 1 ? (float)((H > W ? H : W) - 1) / (float)(out_hw - 1) : 0.f;
  return scale * (TR_T - 1) + 3.f <= (float)TR_P && C >= 1 && C <= 4;
}
hipError_t launch_gather_batch(const uint8_t* codes, const float* lut, const int64_t* rows, int B, int64_t n, int C, int H,
                               int W, int out_hw, const float* vec, const float* future, int L, int T, int stride,
                               const float* mode, float* visual, float* vec_out, float* target, float* mode_out,
                               hipStream_t s) {
  switch (C) {
    case 1: return launch_gather_batch_c<1>(codes, lut, rows, B, n, H, W, out_hw, vec, future, L, T, stride, mode, visual, vec_out, target, mode_out, s);
    case 2: return launch_gather_batch_c<2>(codes, lut, rows, B, n, H, W, out_hw, vec, future, L, T, stride, mode, visual, vec_out, target, mode_out, s);
    case 3: return launch_gather_batch_c<3>(codes, lut, rows, B, n, H, W, out_hw, vec, future, L, T, stride, mode, visual, vec_out, target, mode_out, s);
    case 4: return launch_gather_batch_c<4>(codes, lut, rows, B, n, H, W, out_hw, vec, future, L, T, stride, mode, visual, vec_out, target, mode_out, s);
  }
  return hipErrorInvalidValue;
}

namespace {
__global__ __launch_bounds__(256) void tap_copy_kernel(const void* __restrict__ src, int src_bf16, size_t n,
                                                        float* __restrict__ dst) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256)
    dst[i] = src_bf16 ? __uint_as_float((unsigned)reinterpret_cast<const unsigned short*>(src)[i] << 16)
                      : reinterpret_cast<const float*>(src)[i];
}
}  // namespace

hipError_t launch_tap_copy(const void* src, bool src_bf16, size_t n, float* dst, hipStream_t s) {
  size_t grid = (n + 255) / 256;
  if (grid > 8192) grid = 8192;
  hipLaunchKernelGGL(tap_copy_kernel, dim3((unsigned)grid), dim3(256), 0, s, src, src_bf16 ? 1 : 0, n, dst);
  return hipGetLastError();
}

hipError_t launch_encoder(const EncoderPlan& plan, const float* enc_w, int k0, int kc, const float* visual,
                          const float* vec, int B, float* const bufs[4], float* z, float* feat, int fused_blocks,
                          hipStream_t s, EncoderTap* tap, const unsigned short* enc_wc, size_t wc_stride,
                          const unsigned short* enc_wr, size_t wr_stride) {
  // the tap: after the launch that completes layer `li`, copy its output out and stop
  auto tapped = [&](size_t li) -> bool {
    if (tap == nullptr || tap->layer != (int)li) return false;
    const Layer& l = plan.layers[li];
    const bool pooled = li + 1 == plan.layers.size() && plan.final_hw == 4;
    const size_t n = (size_t)kc * B * (pooled ? 1 : (size_t)l.h_out * l.h_out) * l.cout;
    if (tap->dst != nullptr) (void)launch_tap_copy(bufs[l.dst], false, n, tap->dst, s);
    tap->served = true;
    return true;
  };
  const size_t ms = plan.blob_floats;
  // per layer: 0 = its own launch, 1 = interior of a block, 2 / 3 / 4 = last layer of a block (the block is launched there):
  // 2 = the fp32 fused block of encoder_fused.hip (the leading `fused_blocks`), 3 = a split-f16 tile block, 5 = stem + features.1, 4 = a split-f16
  // row-streaming block (which takes features.2 / 3 over from the fused fp32 kernel when the launch is large enough)
  std::vector<char> in_block(plan.layers.size(), 0);
  std::vector<int> block_of(plan.layers.size(), -1);
  // (development: RIP_SPLIT_TILE_MIN / RIP_SPLIT_ROWS_MIN override the two thresholds, tools/dev/fp32_cross.sh)
  static const int tile_min = getenv("RIP_SPLIT_TILE_MIN") ? atoi(getenv("RIP_SPLIT_TILE_MIN")) : SPLIT_TILE_MIN_PAIRS;
  static const int rows_min = getenv("RIP_SPLIT_ROWS_MIN") ? atoi(getenv("RIP_SPLIT_ROWS_MIN")) : SPLIT_ROWS_MIN_PAIRS;
  const bool split_tiles = enc_wc != nullptr && (long)B * kc >= tile_min;
  const bool split_rows = enc_wr != nullptr && (long)B * kc >= rows_min;
  const bool split_small = enc_wc != nullptr && !split_tiles && tap == nullptr && (long)B * kc >= rows_min;
  for (size_t bi = 0; bi < plan.blocks.size(); ++bi) {
    const FusedBlock& fb = plan.blocks[bi];
    const Layer* le = fb.expand >= 0 ? &plan.layers[fb.expand] : nullptr;
    int how = 0;
    if (split_rows && bi == 0 && fb.expand < 0 && fb.dw == 1 &&
        front_split_supported(plan.layers[0], plan.layers[fb.dw], plan.layers[fb.project])) {
      how = 5;  // stem + features.1 in one kernel: the stem layer is interior to it
      in_block[0] = 1;
    } else if (split_rows && irb_split_rows_supported(le, plan.layers[fb.dw], plan.layers[fb.project])) how = 4;
    else if ((int)bi < fused_blocks) how = 2;
    else if (split_tiles && fb.src != fb.dst && irb_split_tile_supported(le, plan.layers[fb.dw], plan.layers[fb.project])) how = 3;
    if (how == 0) {
      // small launches of the tile-block layers: expansion + depthwise as one launch (launched where the depthwise sits), the
      // projection stays its own layer-wise launch
      if (split_small && le != nullptr && irb_split_tile_supported(le, plan.layers[fb.dw], plan.layers[fb.project])) {
        in_block[fb.expand] = 1;
        in_block[fb.dw] = 6;
        block_of[fb.dw] = (int)bi;
      }
      continue;
    }
    if (fb.expand >= 0) in_block[fb.expand] = 1;
    in_block[fb.dw] = 1;
    in_block[fb.project] = (char)how;  // the block is launched where its last layer sits
    block_of[fb.project] = (int)bi;
  }
  for (size_t li = 0; li < plan.layers.size(); ++li) {
    const Layer& l = plan.layers[li];
    if (in_block[li] == 1) continue;
    if (in_block[li] == 6) {
      const FusedBlock& fb = plan.blocks[block_of[li]];
      hipError_t e = launch_irb_split_expdw(&plan.layers[fb.expand], plan.layers[fb.dw], plan.layers[fb.project],
                                            enc_wc + plan.split_tiles.off[block_of[li]], wc_stride, k0, kc, B, bufs[fb.src], bufs[l.dst], s);
      if (e != hipSuccess) return e;
      continue;
    }
    if (in_block[li] >= 2) {
      const FusedBlock& fb = plan.blocks[block_of[li]];
      const Layer* le = fb.expand >= 0 ? &plan.layers[fb.expand] : nullptr;
      hipError_t e;
      if (in_block[li] == 2)
        e = launch_fused_block(le, plan.layers[fb.dw], plan.layers[fb.project], enc_w, ms, k0, kc, B, bufs[fb.src], bufs[fb.dst], s);
      else if (in_block[li] == 3)
        e = launch_irb_split_tile(le, plan.layers[fb.dw], plan.layers[fb.project], enc_w,
                                  enc_wc + plan.split_tiles.off[block_of[li]], wc_stride, ms, k0, kc, B, bufs[fb.src], bufs[fb.dst], s);
      else if (in_block[li] == 5)
        e = launch_front_split(plan.layers[0], plan.layers[fb.dw], plan.layers[fb.project], enc_w,
                               enc_wr + plan.split_rows.off[block_of[li]], wr_stride, ms, k0, kc, B, visual, bufs[fb.dst], s);
      else
        e = launch_irb_split_rows(le, plan.layers[fb.dw], plan.layers[fb.project], enc_w,
                                  enc_wr + plan.split_rows.off[block_of[li]], wr_stride, ms, k0, kc, B, bufs[fb.src],
                                  bufs[fb.dst], s);
      if (e != hipSuccess) return e;
      if (tapped(li)) return hipGetLastError();
      continue;
    }
    float* dst = bufs[l.dst];
    if (l.kind == L_STEM) {
      const int total = B * l.h_out * l.h_out * 8;
      hipLaunchKernelGGL(stem_kernel, dim3((total + 255) / 256, 1, kc), dim3(256), 0, s, visual, enc_w, ms, k0,
                         l.w_off, l.b_off, B, l.cin, l.h_in, l.h_out, dst);
    } else if (l.kind == L_DW) {
      const long total = (long)B * l.h_out * l.h_out * (l.cout / 4);
      hipLaunchKernelGGL(dw_kernel, dim3((unsigned)((total + 255) / 256), 1, kc), dim3(256), 0, s,
                         (const float*)bufs[l.src], enc_w, ms, k0, l.w_off, l.b_off, B, l.cout, l.h_in, l.h_out,
                         l.stride, dst);
    } else {
      const int M = B * l.h_out * l.h_out;
      const float* res = l.residual ? bufs[l.res] : nullptr;
      const bool pool = li + 1 == plan.layers.size() && plan.final_hw == 4;  // features.18: fuse the 4x4 average pool
      if (pool && split_tiles && head_split_supported(l, plan.final_hw)) {
        hipError_t e = launch_head_split(l, enc_wc + plan.split_tiles.head_off, wc_stride, k0, kc, B, (const float*)bufs[l.src], dst, s);
        if (e != hipSuccess) return e;
      } else {
        dispatch_pw((const float*)bufs[l.src], enc_w, ms, k0, kc, l, res, dst, M, pool, s);
      }
    }
    if (tapped(li)) return hipGetLastError();
  }
  if (tap != nullptr) return hipGetLastError();  // an interior layer of a fused block: not served
  return launch_tail(plan, enc_w, k0, kc, bufs[plan.final_buf], plan.final_hw == 4 ? 1 : plan.final_hw * plan.final_hw, vec,
                     B, bufs[(plan.final_buf + 1) & 3], z, feat, s);
}

// avg-pool + classifier + merger on the fp32 features.18 output `act_last` [kc][B][hw][1280] (hw = 1: already pooled)
hipError_t launch_tail(const EncoderPlan& plan, const float* enc_w, int k0, int kc, const float* act_last, int hw,
                       const float* vec, int B, float* scratch, float* z, float* feat, hipStream_t s) {
  const size_t ms = plan.blob_floats;
  // classifier logits go to `feat` if the caller wants them, else to scratch
  float* feat_buf = feat != nullptr ? feat : scratch;
  if (hw == 1 && B >= 16)
    note_kernel(dim3((B + 15) / 16, kc, FEAT / 16), dim3(256), "cls_mfma_kernel");
  else
    note_kernel(dim3(B, kc, FEAT / CLS_GROUP), dim3(256), "cls_kernel");
  note_kernel(dim3(B, kc), dim3(64), "merger_kernel");
  if (hw == 1 && B >= 16)
    hipLaunchKernelGGL(cls_mfma_kernel, dim3((B + 15) / 16, kc, FEAT / 16), dim3(256), 0, s, act_last, enc_w, ms, k0,
                       plan.cls_w_off, plan.cls_b_off, B, feat_buf);
  else
    hipLaunchKernelGGL(cls_kernel, dim3(B, kc, FEAT / CLS_GROUP), dim3(256), 0, s, act_last,
                       enc_w, ms, k0, plan.cls_w_off, plan.cls_b_off, B, hw, feat_buf);
  hipLaunchKernelGGL(merger_kernel, dim3(B, kc), dim3(64), 0, s, (const float*)feat_buf, enc_w, ms, k0,
                     plan.mrg_w_off[0], plan.mrg_b_off[0], plan.mrg_w_off[1], plan.mrg_b_off[1], plan.mrg_w_off[2],
                     plan.mrg_b_off[2], vec, B, z);
  return hipGetLastError();
}

// ---- the one-launch encoder for small batches (encoder_mega_kernel) ----
namespace {

// pointwise tile shapes of the persistent kernel: the rule of dispatch_pw for ONE model and `want` waves
int mega_pw_variant(int M, const Layer& l, int P, int& ct, int& pt, int& ks) {
  // A layer of the persistent kernel costs (rounds of virtual blocks per workgroup) x (the latency chain of one
  // block), so: as few rounds as the P workgroups allow, the K range split over the block's 4 waves when it is long,
  // and among the shapes with equal rounds the smallest tile (the shortest chain, the most workgroups busy).
  static const int V[8][3] = {{1, 1, 1}, {1, 2, 1}, {2, 2, 1}, {4, 2, 1}, {1, 1, 4}, {1, 2, 4}, {2, 2, 4}, {4, 2, 4}};
  const long n_pt = (M + 15) / 16, n_ct = (l.cout + 15) / 16;
  int best = -1;
  long best_rounds = 0, best_tile = 0;
  for (int v = 0; v < 8; ++v) {
    const int c = V[v][0], p = V[v][1], k = V[v][2];
    if ((k == 4) != (l.cin >= 128)) continue;
    if (c > n_ct && c > 1) continue;
    const long groups = (n_pt + p - 1) / p;
    const long blocks = (k == 1 ? (groups + 3) / 4 : groups) * ((n_ct + c - 1) / c);
    const long rounds = (blocks + P - 1) / P, tile = (long)c * p;
    if (best < 0 || rounds < best_rounds || (rounds == best_rounds && tile < best_tile)) {
      best = v;
      best_rounds = rounds;
      best_tile = tile;
    }
  }
  ct = V[best][0];
  pt = V[best][1];
  ks = V[best][2];
  return best;
}

size_t mega_layout(const EncoderPlan& plan, int B, std::vector<uint32_t>* dst_off, uint32_t* feat_off) {
  size_t off = 0;
  auto take = [&](size_t n) {
    const size_t o = off;
    off += (n + 63) / 64 * 64;  // 256-byte granules: two layers never share a cache line
    return (uint32_t)o;
  };
  const size_t nl = plan.layers.size();
  if (dst_off) dst_off->resize(nl);
  for (size_t li = 0; li < nl; ++li) {
    const Layer& l = plan.layers[li];
    const bool pooled = li + 1 == nl && plan.final_hw == 4;
    const uint32_t o = take(pooled ? (size_t)B * l.cout : (size_t)B * l.h_out * l.h_out * l.cout);
    if (dst_off) (*dst_off)[li] = o;
  }
  const uint32_t f = take((size_t)B * FEAT);
  if (feat_off) *feat_off = f;
  return off;
}

}  // namespace

size_t encoder_mega_arena_floats(const EncoderPlan& plan, int B) { return mega_layout(plan, B, nullptr, nullptr); }

bool encoder_mega_supported(const EncoderPlan& plan, int B, int kc) {
  return (int)plan.layers.size() <= MEGA_MAX_LAYERS && B >= 1 && B <= 16 && kc >= 1 && plan.in_channels <= 16 &&
         (size_t)B * 2500 * 96 < 0xffffffffu;
}

// Is workgroup i of a launch placed on XCD i % 8 on this device (8 XCDs, round-robin)?  Checked once per device.
bool encoder_mega_probe(int device) {
  static int cache[64] = {0};  // 0 unknown, 1 yes, 2 no
  static std::mutex cache_mutex;  // rip_set_option on two handles from two threads
  if (device < 0 || device >= 64) return false;
  std::lock_guard<std::mutex> lock(cache_mutex);
  if (cache[device] != 0) return cache[device] == 1;
  constexpr int G = 256;
  int* d = nullptr;
  bool ok = hipMalloc((void**)&d, G * sizeof(int)) == hipSuccess;
  if (ok) {
    std::vector<int> hst(G, -1);
    for (int rep = 0; rep < 3 && ok; ++rep) {
      // on the NULL stream on purpose: probing from hipStreamPerThread (tried in round 4) left later launches of the
      // one-launch kernel with workgroups off their XCDs (status 1 on every call) — the placement is a property of the
      // queue state, which is why the kernel re-checks it in every launch
      hipLaunchKernelGGL(mega_probe_kernel, dim3(G), dim3(64), 0, 0, d);
      ok = hipMemcpy(hst.data(), d, G * sizeof(int), hipMemcpyDeviceToHost) == hipSuccess;
      for (int i = 0; i < G && ok; ++i) ok = hst[i] == (i & 7);
    }
    (void)hipFree(d);
  }
  cache[device] = ok ? 1 : 2;
  return ok;
}

hipError_t launch_encoder_mega(const EncoderPlan& plan, const float* enc_w, int k0, int kc, const float* visual,
                               const float* vec, int B, float* arena, size_t arena_model_stride, unsigned* sync,
                               int* status, unsigned long long* ticks, float* z, float* feat, int wgs_per_xcd,
                               hipStream_t s) {
  MegaArgs a;
  std::memset(&a, 0, sizeof(a));
  std::vector<uint32_t> dst_off;
  uint32_t feat_off = 0;
  mega_layout(plan, B, &dst_off, &feat_off);
  // where each of the four rotating workspace ids of the plan was last written
  uint32_t where[4] = {MEGA_NONE, MEGA_NONE, MEGA_NONE, MEGA_NONE};
  const int P = wgs_per_xcd;
  const size_t nl = plan.layers.size();
  for (size_t li = 0; li < nl; ++li) {
    const Layer& l = plan.layers[li];
    MegaLayer& L = a.layers[li];
    L.w_off = (uint32_t)l.w_off;
    L.b_off = (uint32_t)l.b_off;
    L.src = l.src < 0 ? MEGA_NONE : where[l.src];
    L.res = l.residual ? where[l.res] : MEGA_NONE;
    L.dst = dst_off[li];
    L.cin = (uint16_t)l.cin;
    L.cout = (uint16_t)l.cout;
    L.kind = (uint8_t)l.kind;
    L.h_in = (uint8_t)l.h_in;
    L.h_out = (uint8_t)l.h_out;
    L.stride = (uint8_t)l.stride;
    L.gy = 1;
    if (l.kind == L_STEM) {
      L.gx = (uint16_t)(((long)B * l.h_out * l.h_out * 8 + 255) / 256);
    } else if (l.kind == L_DW) {
      L.gx = (uint16_t)(((long)B * l.h_out * l.h_out * (l.cout / 4) + 255) / 256);
    } else {
      const int M = B * l.h_out * l.h_out;
      const bool pool = li + 1 == nl && plan.final_hw == 4;
      int ct = 1, pt = 1, ks = 1;
      L.variant = (uint8_t)mega_pw_variant(M, l, P, ct, pt, ks);
      const int n_pt = (M + 15) / 16, n_ct = (l.cout + 15) / 16, groups = (n_pt + pt - 1) / pt;
      L.gx = (uint16_t)(ks == 1 ? (groups + 3) / 4 : groups);
      L.gy = (uint16_t)((n_ct + ct - 1) / ct);
      L.M = (uint32_t)M;
      L.flags = (uint8_t)(l.relu6 | (pool ? 2 : 0));
    }
    where[l.dst] = L.dst;
  }
  a.n_layers = (int)nl;
  a.visual = visual;
  a.vec = vec;
  a.wbase = enc_w;
  a.arena = arena;
  a.z = z;
  a.feat = feat;
  a.sync = sync;
  a.status = status;
  a.ticks = ticks;
  a.model_stride = plan.blob_floats;
  a.arena_model_stride = arena_model_stride;
  a.cls_w = plan.cls_w_off;
  a.cls_b = plan.cls_b_off;
  a.m0w = plan.mrg_w_off[0];
  a.m0b = plan.mrg_b_off[0];
  a.m1w = plan.mrg_w_off[1];
  a.m1b = plan.mrg_b_off[1];
  a.m2w = plan.mrg_w_off[2];
  a.m2b = plan.mrg_b_off[2];
  a.last_off = dst_off[nl - 1];
  a.feat_off = feat_off;
  a.last_hw = plan.final_hw == 4 ? 1 : plan.final_hw * plan.final_hw;
  a.k0 = k0;
  a.kc = kc;
  a.B = B;
  a.C = plan.in_channels;
  hipLaunchKernelGGL(encoder_mega_kernel, dim3(8 * P), dim3(256), 0, s, a);
  return hipGetLastError();
}

}  // namespace rip
