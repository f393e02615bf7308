// LIDAR point cloud -> bird's-eye-view occupancy histogram for gfx950 (the step that produces the
// `lidar` observation the hot path starts from).
//
// Reference: carla_lidar_measurement_to_ndarray (oatomobile/utils/carla.py:165-233): the [P,3] float32 points are split at
// z = -2.5 m into a `below` (z <= -2.5) and an `above` (z >= -2.5) cloud, each is histogrammed over (x, y) with
// np.histogramdd on the float64 edges np.linspace(-50, 51, 201) (200 bins of 0.505 m), counts are clipped at 5 and
// divided by 5; result float32 [200, 200, 2].  Integer work, bit-exact against the reference (tests/golden/g9_lidar.npz).
//
// Mapping: one workgroup of 1024 threads per observation; the 200x200 counters of ONE height channel live in LDS as
// 16-bit halves of 32-bit words (80 KB), the clipped result of the first channel is parked as bytes (40 KB) while the
// second channel is counted (the point list is read twice, the second time from L2), then both channels are written as
// one coalesced float2 per cell.  HBM traffic = 12 B per point + 320 KB per observation, no global atomics.
//
// Bin rule = numpy's: searchsorted(edges, x, side="right") - 1 on the float64 edge table, last bin closed on the right,
// outliers / NaN dropped.  The table is built on the host with numpy's own formula (arange * step + start, last = stop;
// two roundings, no FMA) and the kernel fixes up an arithmetic guess against it, so the result does not depend on how
// the device rounds the guess.
#include <hip/hip_runtime.h>

#include "flow.h"

namespace rip {

namespace {

constexpr int BEV = 200;               // bins per axis
constexpr int CELLS = BEV * BEV;       // 40 000
constexpr int BEV_THREADS = 1024;
constexpr int HIST_MAX = 5;

__constant__ double c_edges[BEV + 1];

// `e`: the edge table in LDS (per-lane indices: from constant memory this is a divergent vector load per look-up)
__device__ __forceinline__ int bev_bin(float v, const double* e) {
  const double x = (double)v;
  if (!(x >= -50.0) || !(x <= 51.0)) return -1;  // outliers and NaN (both comparisons false); e[0], e[200] are exact
  if (x == 51.0) return BEV - 1;                 // the last bin is closed on the right
  int g = (int)((x + 50.0) * (200.0 / 101.0));
  g = g < 0 ? 0 : (g > BEV - 1 ? BEV - 1 : g);
  // the guess is off by at most one: a single conditional step each way, checked against the table
  g -= (g > 0 && x < e[g]) ? 1 : 0;
  g += (g < BEV - 1 && x >= e[g + 1]) ? 1 : 0;
  g -= (g > 0 && x < e[g]) ? 1 : 0;
  return g;
}

__global__ __launch_bounds__(BEV_THREADS) void lidar_bev_kernel(const float* __restrict__ points,
                                                                 const int* __restrict__ offsets,
                                                                 float* __restrict__ bev) {
  __shared__ unsigned cnt[CELLS / 2];       // two 16-bit counters per word
  __shared__ unsigned char first[CELLS];    // clipped counts of channel 0
  __shared__ double edges[BEV + 1];
  const int b = blockIdx.x, tid = threadIdx.x;
  if (tid <= BEV) edges[tid] = c_edges[tid];
  const int p0 = offsets[b], p1 = offsets[b + 1];
  for (int ch = 0; ch < 2; ++ch) {
    for (int i = tid; i < CELLS / 2; i += BEV_THREADS) cnt[i] = 0u;
    __syncthreads();
    for (int p = p0 + tid; p < p1; p += BEV_THREADS) {
      const float x = points[(size_t)p * 3], y = points[(size_t)p * 3 + 1], z = points[(size_t)p * 3 + 2];
      const bool take = ch == 0 ? (z <= -2.5f) : (z >= -2.5f);  // utils/carla.py:216-217 (z == -2.5 counts in both)
      if (!take) continue;
      const int bx = bev_bin(x, edges), by = bev_bin(y, edges);
      if (bx < 0 || by < 0) continue;
      const int cell = bx * BEV + by;
      const unsigned sh = 16u * (cell & 1);
      // counts saturate at the clip: a cell is left alone once it shows >= 5, so a 16-bit half can never carry
      // (at most 5 + one increment per thread already past the check)
      if (((cnt[cell >> 1] >> sh) & 0xffffu) < (unsigned)HIST_MAX) atomicAdd(&cnt[cell >> 1], 1u << sh);
    }
    __syncthreads();
    if (ch == 0) {
      for (int c = tid; c < CELLS; c += BEV_THREADS) {
        const unsigned v = (cnt[c >> 1] >> (16u * (c & 1))) & 0xffffu;
        first[c] = (unsigned char)(v > HIST_MAX ? HIST_MAX : v);
      }
      __syncthreads();
    }
  }
  // hist / 5 in float64, then float32 (utils/carla.py:205, :233): k / 5 for k = 0..5
  const float lut[HIST_MAX + 1] = {0.0f, (float)(1.0 / 5.0), (float)(2.0 / 5.0), (float)(3.0 / 5.0), (float)(4.0 / 5.0), 1.0f};
  float2* out = reinterpret_cast<float2*>(bev) + (size_t)b * CELLS;
  for (int c = tid; c < CELLS; c += BEV_THREADS) {
    const unsigned v = (cnt[c >> 1] >> (16u * (c & 1))) & 0xffffu;
    out[c] = make_float2(lut[first[c]], lut[v > HIST_MAX ? HIST_MAX : v]);
  }
}

// ---------------------------------------------------------------------------------------------------------
// Hindsight labelling of a recording (CARLADataset.process, oatomobile/datasets/carla.py:237-325): every window
// (frame i, its P predecessors, its L successors) of a pose track -> player_past / player_future in frame i's ego
// frame (world2local, utils/carla.py:642-674) and the targets derived from the future (future.npy / goal.npy /
// mode.npy of the packed cache).  One workgroup per window: wave 0's first lane builds the float64 rotation matrix
// ('sxyz' euler2mat(roll, pitch, yaw).T from deg2rad of the float32 angles) into LDS, then one lane per waypoint
// subtracts in float32 (both operands are float32 sensor outputs: what numpy does) and multiplies in float64.
// 24 B read + 24-32 B written per waypoint: the launch is latency-bound at any real size.
// ---------------------------------------------------------------------------------------------------------
constexpr int HS_THREADS = 128;

struct HindsightArgs {
  const float* location;   // [N,3]
  const float* rotation;   // [N,3] (pitch, yaw, roll) degrees
  const int* episode;      // [N]
  const int* frames;       // [M]
  int N, M, L, P, G, goal_stride;
  double* future64;        // [M,L,3] or null
  double* past64;          // [M,P,3] or null
  float* future_xy;        // [M,L,2] or null
  float* goal;             // [M,G,2] or null
  float* mode;             // [M] or null
  unsigned char* valid;    // [M] or null
};

// row `f` of the window around frame i (f = the absolute frame index) in i's ego frame
__device__ __forceinline__ void hs_local(const float* __restrict__ location, const float cur[3], const double* R, int f,
                                         double out[3]) {
#pragma clang fp contract(off)
  const float dx = location[(size_t)f * 3] - cur[0], dy = location[(size_t)f * 3 + 1] - cur[1],
              dz = location[(size_t)f * 3 + 2] - cur[2];
  for (int r = 0; r < 3; ++r) out[r] = R[r * 3] * (double)dx + R[r * 3 + 1] * (double)dy + R[r * 3 + 2] * (double)dz;
}

// datasets/carla.py:148-162 on the float32 waypoint, as load_datum(mode=True) computes it (theta <= -15 cannot occur)
__device__ __forceinline__ float hs_mode(float x, float y) {
#pragma clang fp contract(off)
  const float norm = sqrtf(x * x + y * y);
  const float theta = acosf(x / (norm + 1e-3f)) * (float)(180.0 / 3.14159265358979323846);
  return norm < 3.0f ? 1.0f : (theta > 15.0f ? 2.0f : 0.0f);
}

__global__ __launch_bounds__(HS_THREADS) void hindsight_targets_kernel(HindsightArgs a) {
#pragma clang fp contract(off)
  __shared__ double R[9];
  const int tid = threadIdx.x;
  const double nan64 = __longlong_as_double(0x7ff8000000000000LL);
  const float nan32 = __int_as_float(0x7fc00000);
  for (int m = blockIdx.x; m < a.M; m += gridDim.x) {
    const int i = a.frames[m];
    // the range test comes first: nothing outside [0, N) is read, the episode numbers included
    bool ok = i >= a.P && i < a.N - a.L;
    if (ok) {
      const int e = a.episode[i];
      ok = a.episode[i - a.P] == e && a.episode[i + a.L] == e;
    }
    float cur[3] = {0.f, 0.f, 0.f};
    if (ok) {
      for (int c = 0; c < 3; ++c) cur[c] = a.location[(size_t)i * 3 + c];
      if (tid == 0) {
        const double d2r = 3.14159265358979323846 / 180.0;  // numpy's deg2rad: x * (pi / 180)
        const double pitch = (double)a.rotation[(size_t)i * 3] * d2r, yaw = (double)a.rotation[(size_t)i * 3 + 1] * d2r,
                     roll = (double)a.rotation[(size_t)i * 3 + 2] * d2r;
        const double ci = cos(roll), si = sin(roll), cj = cos(pitch), sj = sin(pitch), ck = cos(yaw), sk = sin(yaw);
        const double cc = ci * ck, cs = ci * sk, sc = si * ck, ss = si * sk;
        // euler2mat rows (cj*ck, sj*sc-cs, sj*cc+ss), (cj*sk, sj*ss+cc, sj*cs-sc), (-sj, cj*si, cj*ci), transposed
        R[0] = cj * ck;      R[1] = cj * sk;      R[2] = -sj;
        R[3] = sj * sc - cs; R[4] = sj * ss + cc; R[5] = cj * si;
        R[6] = sj * cc + ss; R[7] = sj * cs - sc; R[8] = cj * ci;
      }
    }
    __syncthreads();
    const size_t mL = (size_t)m * a.L, mP = (size_t)m * a.P;
    for (int j = tid; j < a.P + a.L; j += HS_THREADS) {
      const bool past = j < a.P;
      const int row = past ? j : j - a.P;                    // past row j = frame i - P + j, future row j = frame i + 1 + j
      double v[3] = {nan64, nan64, nan64};
      if (ok) hs_local(a.location, cur, R, past ? i - a.P + j : i + 1 + row, v);
      if (past) {
        if (a.past64 != nullptr)
          for (int c = 0; c < 3; ++c) a.past64[(mP + row) * 3 + c] = v[c];
      } else {
        if (a.future64 != nullptr)
          for (int c = 0; c < 3; ++c) a.future64[(mL + row) * 3 + c] = v[c];
        if (a.future_xy != nullptr)
          reinterpret_cast<float2*>(a.future_xy)[mL + row] = make_float2((float)v[0], (float)v[1]);
        if (row == a.L - 1) {
          if (a.mode != nullptr) a.mode[m] = ok ? hs_mode((float)v[0], (float)v[1]) : nan32;
          if (a.valid != nullptr) a.valid[m] = ok ? 1 : 0;
        }
      }
    }
    if (a.goal != nullptr) {
      // goal_from_future: future rows stride-1, 2*stride-1, ... (L / stride of them), the last one repeated up to G
      const int have = a.L / a.goal_stride;  // >= 1: checked by the entry point
      for (int g = tid; g < a.G; g += HS_THREADS) {
        const int row = ((g < have ? g : have - 1) + 1) * a.goal_stride - 1;
        double v[3] = {nan64, nan64, nan64};
        if (ok) hs_local(a.location, cur, R, i + 1 + row, v);
        reinterpret_cast<float2*>(a.goal)[(size_t)m * a.G + g] = make_float2((float)v[0], (float)v[1]);
      }
    }
    __syncthreads();  // R is rebuilt by the next window of this workgroup
  }
}

// ---------------------------------------------------------------------------------------------------------
// _datum.code_bev against a FIXED table: the float32 BEV read as uint32 bit patterns (-0.0 and +0.0 stay apart) ->
// the uint8 index of each cell's pattern in `table` (ascending, n <= 256; held in LDS padded to 256 entries so that
// the lower bound is eight unconditional halvings).  A pattern that is not in the table, and every NaN, codes as 0
// and counts into *miss: summed per workgroup in LDS, one global atomic add per workgroup that saw any.  16-byte loads
// and 4-byte packed stores over the groups of four cells, the (total % 4) cells left over one per lane.
// 5 B per cell: 400 KB per 200 x 200 x 2 observation, a few microseconds of HBM time under the launch latency.
// ---------------------------------------------------------------------------------------------------------
constexpr int CODE_THREADS = 256;

__device__ __forceinline__ unsigned code_of(unsigned x, const unsigned* tab, int n, unsigned& misses) {
  unsigned lo = 0;
#pragma unroll
  for (unsigned step = 128; step; step >>= 1) lo += (tab[lo + step - 1] < x) ? step : 0u;  // lo <= 255
  const bool hit = (int)lo < n && tab[lo] == x && (x & 0x7fffffffu) <= 0x7f800000u;
  misses += hit ? 0u : 1u;
  return hit ? lo : 0u;
}

// `groups` = cells / 4 when both pointers allow the wide accesses, else 0 (every cell goes one per lane)
__global__ __launch_bounds__(CODE_THREADS) void code_bev_u8_kernel(const unsigned* __restrict__ bits, long long cells,
                                                                    long long groups, const unsigned* __restrict__ table,
                                                                    int n, unsigned char* __restrict__ codes,
                                                                    unsigned* __restrict__ miss) {
  __shared__ unsigned tab[256];
  __shared__ unsigned s_miss;
  const int tid = threadIdx.x;
  tab[tid] = tid < n ? table[tid] : 0xffffffffu;
  if (tid == 0) s_miss = 0u;
  __syncthreads();
  unsigned misses = 0u;
  const long long stride = (long long)gridDim.x * CODE_THREADS;
  const long long first = (long long)blockIdx.x * CODE_THREADS + tid;
  for (long long g = first; g < groups; g += stride) {
    const uint4 v = reinterpret_cast<const uint4*>(bits)[g];
    const unsigned c = code_of(v.x, tab, n, misses) | (code_of(v.y, tab, n, misses) << 8) |
                       (code_of(v.z, tab, n, misses) << 16) | (code_of(v.w, tab, n, misses) << 24);
    reinterpret_cast<unsigned*>(codes)[g] = c;
  }
  for (long long c = groups * 4 + first; c < cells; c += stride) codes[c] = (unsigned char)code_of(bits[c], tab, n, misses);
  if (misses) atomicAdd(&s_miss, misses);
  __syncthreads();
  if (tid == 0 && s_miss) atomicAdd(miss, s_miss);
}

}  // namespace

hipError_t launch_hindsight_targets(const float* location, const float* rotation, const int* episode, int N,
                                    const int* frames, int M, int L, int P, int G, int goal_stride, double* future64,
                                    double* past64, float* future_xy, float* goal, float* mode, unsigned char* valid,
                                    hipStream_t s) {
  if (M <= 0) return hipSuccess;
  HindsightArgs a{location, rotation, episode, frames, N, M, L, P, G, goal_stride, future64, past64, future_xy, goal, mode, valid};
  hipLaunchKernelGGL(hindsight_targets_kernel, dim3(M < 65536 ? M : 65536), dim3(HS_THREADS), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_code_bev_u8(const float* bev, long long cells, const unsigned* table, int n_values, unsigned char* codes,
                              unsigned* miss, hipStream_t s) {
  if (cells <= 0) return hipSuccess;
  const bool wide = (reinterpret_cast<uintptr_t>(bev) & 15u) == 0 && (reinterpret_cast<uintptr_t>(codes) & 3u) == 0;
  const long long groups = wide ? cells / 4 : 0;
  const long long work = groups + (cells - groups * 4);
  long long blocks = (work + CODE_THREADS - 1) / CODE_THREADS;
  blocks = blocks < 1 ? 1 : (blocks > 2048 ? 2048 : blocks);
  hipLaunchKernelGGL(code_bev_u8_kernel, dim3((unsigned)blocks), dim3(CODE_THREADS), 0, s,
                     reinterpret_cast<const unsigned*>(bev), cells, groups, table, n_values, codes, miss);
  return hipGetLastError();
}

hipError_t launch_lidar_bev(const float* points, const int* offsets, int B, float* bev, hipStream_t s) {
  static bool edges_ready[64] = {false};
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return e;
  if (dev < 0 || dev >= 64) return hipErrorInvalidDevice;
  if (!edges_ready[dev]) {
#pragma clang fp contract(off)
    double edges[BEV + 1];
    const double start = -50.0, stop = 51.0;
    const double step = (stop - start) / (double)BEV;  // numpy.linspace: delta / div
    for (int i = 0; i <= BEV; ++i) {
      const double m = (double)i * step;  // arange(0, num) * step
      edges[i] = m + start;               // + start
    }
    edges[BEV] = stop;                     // endpoint
    e = hipMemcpyToSymbol(HIP_SYMBOL(c_edges), edges, sizeof(edges));
    if (e != hipSuccess) return e;
    edges_ready[dev] = true;
  }
  if (B <= 0) return hipSuccess;
  hipLaunchKernelGGL(lidar_bev_kernel, dim3(B), dim3(BEV_THREADS), 0, s, points, offsets, bev);
  return hipGetLastError();
}

}  // namespace rip
