// Producers of FP8 activations for the W8A8 GEMM (gemm_fp8.hip), gfx950:
//   * per-row dynamic quantisation of a 16-bit matrix to OCP e4m3fn bytes,
//   * RMSNorm (+ fused residual add) whose normalised f32 row is quantised
//     directly -- no 16-bit rounding and no second kernel in between.
// scale[row] = amax(|row|) / 448 (1 for an all-zero row), q = x / scale clamped
// to +-448 BEFORE the conversion (the packed convert is not relied on to
// saturate).  norm.hip's half-wave-per-row layout: 32 lanes own a row, a lane
// owns 16 consecutive elements per 512-element pass, so it loads 2 x 16 B and
// stores 16 B of fp8; the row reductions stay inside the half wave.
#include "common.h"
#include <stdexcept>

namespace rdb {

namespace {

constexpr float kFp8Max = 448.0f;   // largest finite e4m3fn

template <typename T>
__device__ __forceinline__ void q_load16(const T* p, float* o) {
  const u32x4 r0 = *reinterpret_cast<const u32x4*>(p);
  const u32x4 r1 = *reinterpret_cast<const u32x4*>(p + 8);
  const T* e0 = reinterpret_cast<const T*>(&r0);
  const T* e1 = reinterpret_cast<const T*>(&r1);
#pragma unroll
  for (int q = 0; q < 8; ++q) { o[q] = (float)e0[q]; o[8 + q] = (float)e1[q]; }
}
template <typename T>
__device__ __forceinline__ void q_store16(T* p, const float* o) {
  T v[16];
#pragma unroll
  for (int q = 0; q < 16; ++q) v[q] = (T)o[q];
  reinterpret_cast<u32x4*>(p)[0] = reinterpret_cast<const u32x4*>(v)[0];
  reinterpret_cast<u32x4*>(p)[1] = reinterpret_cast<const u32x4*>(v)[1];
}
__device__ __forceinline__ float half_max(float v) {
#pragma unroll
  for (int o = 16; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ float half_add(float v) {
#pragma unroll
  for (int o = 16; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ float amax16(const float* v, float am) {
#pragma unroll
  for (int q = 0; q < 16; ++q) am = fmaxf(am, fabsf(v[q]));
  return am;
}
// 16 f32 -> 16 e4m3fn bytes (v_cvt_pk_fp8_f32: OCP format on gfx950, RNE), one 16-B store
__device__ __forceinline__ void store_fp8x16(uint8_t* p, const float* v, float sc) {
  u32x4 out;
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    float c[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) c[e] = fminf(fmaxf(v[4 * w + e] / sc, -kFp8Max), kFp8Max);
    int pk = 0;
    pk = __builtin_amdgcn_cvt_pk_fp8_f32(c[0], c[1], pk, false);
    pk = __builtin_amdgcn_cvt_pk_fp8_f32(c[2], c[3], pk, true);
    out[w] = (uint32_t)pk;
  }
  *reinterpret_cast<u32x4*>(p) = out;
}

// Half wave per row, any K % 16 == 0 (short rows, and rows past the block form's
// 16384): the row is read twice, the second pass hits L2 / L1.
template <typename T>
__global__ void __launch_bounds__(256)
quant_rows_kernel(const T* __restrict__ x, uint8_t* __restrict__ q, float* __restrict__ scale, int rows, int K,
                  int ldx) {
  const int hl = threadIdx.x & 31;
  const int row = blockIdx.x * 8 + (threadIdx.x >> 5);
  if (row >= rows) return;      // whole half waves only
  const T* xr = x + (size_t)row * ldx;
  float am = 0.f;
  for (int c = hl * 16; c < K; c += 512) {
    float v[16];
    q_load16(xr + c, v);
    am = amax16(v, am);
  }
  am = half_max(am);
  const float sc = am > 0.f ? am / kFp8Max : 1.0f;
  if (hl == 0) scale[row] = sc;
  uint8_t* qr = q + (size_t)row * K;
  for (int c = hl * 16; c < K; c += 512) {
    float v[16];
    q_load16(xr + c, v);
    store_fp8x16(qr + c, v, sc);
  }
}

// RMSNorm + quantise, half wave per row (D < 1024): rows of up to 512 * NV elements stay in
// registers (f32) between the sum of squares, the amax of the normalised row and the store.
template <typename T, int NV>
__global__ void __launch_bounds__(256)
rms_quant_kernel(const T* __restrict__ x, const T* __restrict__ res, T* __restrict__ res_out,
                 const T* __restrict__ gamma, uint8_t* __restrict__ q, float* __restrict__ scale, int rows, int D,
                 int ldx, float eps) {
  const int hl = threadIdx.x & 31;
  const int row = blockIdx.x * 8 + (threadIdx.x >> 5);
  if (row >= rows) return;
  const T* xr = x + (size_t)row * ldx;
  float v[NV][16];
  float ss = 0.f;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int c = i * 512 + hl * 16;
    if (c < D) {
      q_load16(xr + c, v[i]);
      if (res != nullptr) {
        float r[16];
        q_load16(res + (size_t)row * D + c, r);
#pragma unroll
        for (int e = 0; e < 16; ++e) v[i][e] += r[e];
        if (res_out != nullptr) q_store16(res_out + (size_t)row * D + c, v[i]);
      }
    } else {
#pragma unroll
      for (int e = 0; e < 16; ++e) v[i][e] = 0.f;
    }
#pragma unroll
    for (int e = 0; e < 16; ++e) ss += v[i][e] * v[i][e];
  }
  const float rstd = rsqrtf(half_add(ss) * (1.0f / D) + eps);
  float am = 0.f;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int c = i * 512 + hl * 16;
    if (c < D) {
      float g[16];
      q_load16(gamma + c, g);
#pragma unroll
      for (int e = 0; e < 16; ++e) v[i][e] = v[i][e] * rstd * g[e];
      am = amax16(v[i], am);
    }
  }
  am = half_max(am);
  const float sc = am > 0.f ? am / kFp8Max : 1.0f;
  if (hl == 0) scale[row] = sc;
  uint8_t* qr = q + (size_t)row * D;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int c = i * 512 + hl * 16;
    if (c < D) store_fp8x16(qr + c, v[i], sc);
  }
}

// Block-per-row forms for long rows (K >= 1024): at the prefill sizes (128 .. 1024
// rows) eight rows per block leave most CUs idle and a half wave walks its row
// in a chain of dependent-latency passes.  Here 256 threads share one row, a
// thread owns 16 consecutive elements per 4096-element pass (still 2 x 16-B
// loads, one 16-B store), the row is read once, and the two reductions cross
// the four waves through LDS.
__device__ __forceinline__ float block_max(float v, float* sh) {
  v = wave_max(v);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  v = fmaxf(fmaxf(sh[0], sh[1]), fmaxf(sh[2], sh[3]));
  __syncthreads();
  return v;
}
__device__ __forceinline__ float block_add(float v, float* sh) {
  v = wave_sum(v);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  v = (sh[0] + sh[1]) + (sh[2] + sh[3]);
  __syncthreads();
  return v;
}

template <typename T, int NP>
__global__ void __launch_bounds__(256)
quant_row_block_kernel(const T* __restrict__ x, uint8_t* __restrict__ q, float* __restrict__ scale, int K, int ldx) {
  __shared__ float sh[4];
  const int row = blockIdx.x;
  const T* xr = x + (size_t)row * ldx;
  u32x4 raw[NP][2];
  float am = 0.f;
#pragma unroll
  for (int p = 0; p < NP; ++p) {
    const int c = p * 4096 + threadIdx.x * 16;
    if (c < K) {
      raw[p][0] = *reinterpret_cast<const u32x4*>(xr + c);
      raw[p][1] = *reinterpret_cast<const u32x4*>(xr + c + 8);
    } else {
      raw[p][0] = raw[p][1] = u32x4{0u, 0u, 0u, 0u};
    }
    const T* e = reinterpret_cast<const T*>(raw[p]);
#pragma unroll
    for (int i = 0; i < 16; ++i) am = fmaxf(am, fabsf((float)e[i]));
  }
  am = block_max(am, sh);
  const float sc = am > 0.f ? am / kFp8Max : 1.0f;
  if (threadIdx.x == 0) scale[row] = sc;
  uint8_t* qr = q + (size_t)row * K;
#pragma unroll
  for (int p = 0; p < NP; ++p) {
    const int c = p * 4096 + threadIdx.x * 16;
    if (c < K) {
      const T* e = reinterpret_cast<const T*>(raw[p]);
      float v[16];
#pragma unroll
      for (int i = 0; i < 16; ++i) v[i] = (float)e[i];
      store_fp8x16(qr + c, v, sc);
    }
  }
}

// D <= 4096: one pass, the row lives in 16 f32 registers per thread
template <typename T>
__global__ void __launch_bounds__(256)
rms_quant_block_kernel(const T* __restrict__ x, const T* __restrict__ res, T* __restrict__ res_out,
                       const T* __restrict__ gamma, uint8_t* __restrict__ q, float* __restrict__ scale, int D, int ldx,
                       float eps) {
  __shared__ float sh[4];
  const int row = blockIdx.x;
  const int c = threadIdx.x * 16;
  const bool on = c < D;
  float v[16], g[16];
#pragma unroll
  for (int e = 0; e < 16; ++e) v[e] = g[e] = 0.f;
  if (on) {
    q_load16(x + (size_t)row * ldx + c, v);
    q_load16(gamma + c, g);
    if (res != nullptr) {
      float r[16];
      q_load16(res + (size_t)row * D + c, r);
#pragma unroll
      for (int e = 0; e < 16; ++e) v[e] += r[e];
      if (res_out != nullptr) q_store16(res_out + (size_t)row * D + c, v);
    }
  }
  float ss = 0.f;
#pragma unroll
  for (int e = 0; e < 16; ++e) ss += v[e] * v[e];
  const float rstd = rsqrtf(block_add(ss, sh) * (1.0f / D) + eps);
#pragma unroll
  for (int e = 0; e < 16; ++e) v[e] = v[e] * rstd * g[e];
  const float am = block_max(amax16(v, 0.f), sh);
  const float sc = am > 0.f ? am / kFp8Max : 1.0f;
  if (threadIdx.x == 0) scale[row] = sc;
  if (on) store_fp8x16(q + (size_t)row * D + c, v, sc);
}

template <typename T>
void launch_quant_rows(hipStream_t s, uintptr_t x, int ldx, uintptr_t q, uintptr_t scale, int rows, int K) {
  const dim3 blk(256);
  if (K >= 1024 && K <= 16384) {
    const dim3 grid(rows);
#define RDB_QB(NP)                                                                                              \
  if (K <= 4096 * NP) {                                                                                         \
    hipLaunchKernelGGL((quant_row_block_kernel<T, NP>), grid, blk, 0, s, (const T*)x, (uint8_t*)q, (float*)scale, K, \
                       ldx);                                                                                    \
    return;                                                                                                     \
  }
    RDB_QB(1) RDB_QB(2) RDB_QB(4)
#undef RDB_QB
  }
  hipLaunchKernelGGL(quant_rows_kernel<T>, dim3((rows + 7) / 8), blk, 0, s, (const T*)x, (uint8_t*)q, (float*)scale,
                     rows, K, ldx);
}

template <typename T>
void launch_rms_quant(hipStream_t s, uintptr_t x, uintptr_t res, uintptr_t res_out, uintptr_t gamma, uintptr_t q,
                      uintptr_t scale, int rows, int D, int ldx, float eps) {
  const dim3 grid((rows + 7) / 8), blk(256);
  if (D >= 1024) {
    hipLaunchKernelGGL(rms_quant_block_kernel<T>, dim3(rows), blk, 0, s, (const T*)x, (const T*)res, (T*)res_out,
                       (const T*)gamma, (uint8_t*)q, (float*)scale, D, ldx, eps);
    return;
  }
  const int need = (D + 511) / 512;
#define RDB_RQ(NV)                                                                                            \
  if (need <= NV) {                                                                                            \
    hipLaunchKernelGGL((rms_quant_kernel<T, NV>), grid, blk, 0, s, (const T*)x, (const T*)res, (T*)res_out,    \
                       (const T*)gamma, (uint8_t*)q, (float*)scale, rows, D, ldx, eps);                        \
    return;                                                                                                    \
  }
  RDB_RQ(1) RDB_RQ(2)
#undef RDB_RQ
}

}  // namespace

void quant_fp8_rows(int dtype, uintptr_t x, int ldx, uintptr_t q, uintptr_t scale, int rows, int K,
                    uintptr_t stream) {
  if (K <= 0 || K % 16 != 0) throw std::invalid_argument("quant_fp8_rows: K must be a positive multiple of 16");
  if (ldx < K || ldx % 8 != 0 || ((x | q) & 15) || (scale & 3))
    throw std::invalid_argument("quant_fp8_rows: rows must be 16-byte aligned");
  if (rows <= 0) return;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (dtype == 0) launch_quant_rows<bf16>(s, x, ldx, q, scale, rows, K);
  else if (dtype == 1) launch_quant_rows<f16>(s, x, ldx, q, scale, rows, K);
  else
    throw std::invalid_argument("quant_fp8_rows: dtype must be bf16 or f16");
  RDB_HIP_CHECK(hipGetLastError());
}

void rms_norm_fp8(int dtype, uintptr_t x, uintptr_t res, uintptr_t res_out, uintptr_t gamma, uintptr_t q,
                  uintptr_t scale, int rows, int D, int ldx, float eps, uintptr_t stream) {
  if (D <= 0 || D % 16 != 0 || D > 4096) throw std::invalid_argument("rms_norm_fp8: D must be a multiple of 16, <= 4096");
  if (ldx < D || ldx % 8 != 0 || (ldx != D && res != 0)) throw std::invalid_argument("rms_norm_fp8: bad x row stride");
  if (((x | res | res_out | gamma | q) & 15) || (scale & 3))
    throw std::invalid_argument("rms_norm_fp8: operands must be 16-byte aligned");
  if (rows <= 0) return;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (dtype == 0) launch_rms_quant<bf16>(s, x, res, res_out, gamma, q, scale, rows, D, ldx, eps);
  else if (dtype == 1) launch_rms_quant<f16>(s, x, res, res_out, gamma, q, scale, rows, D, ldx, eps);
  else throw std::invalid_argument("rms_norm_fp8: dtype must be bf16 or f16");
  RDB_HIP_CHECK(hipGetLastError());
}

}  // namespace rdb
