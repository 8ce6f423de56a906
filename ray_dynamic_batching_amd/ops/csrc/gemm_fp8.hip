// W8A8 GEMM for gfx950: e4m3 (OCP) activations and weights, f32 accumulation,
// per-row / per-output-channel f32 scales applied in the epilogue:
//   C[M,N] = act( (Aq[M,K] . Wq[N,K]^T) * sa[m] * sw[n] + bias[n] ) + residual
// Main loop: both operands are staged global -> LDS with 16-byte LDS-DMA loads
// (STAGES buffers, counted vmcnt + raw s_barrier: the bf16 kernels' protocol),
// read back as 2 x ds_read_b128 per 16-row fragment and multiplied with the
// block-scaled v_mfma_scale_f32_16x16x128_f8f6f4 at hardware scales of 1.0
// (twice the bf16 MFMA rate; half the staged bytes per FLOP of a bf16 tile).
//
// One K step is 128 bytes per row, so the LDS image has the bf16 kernels'
// geometry: 128-B rows, a DMA instruction writes 8 rows x 8 chunks linearly and
// the swizzle is applied on the SOURCE side.  The key differs from gemm_core.h's
// swz_off: a lane of the K = 128 MFMA reads chunks 2*(lane >> 4) and
// 2*(lane >> 4) + 1, and the ds_read_b128 lane groups ({0-3, 12-15, 20-27},
// {4-11, 16-19, 28-31}, + 32) mix rows {0-3, 12-15} of one k quarter with rows
// {4-11} of the next, i.e. chunk c with chunk c ^ 2.  swz_key sends the row
// pairs of {4-11} to even keys and the others to odd keys, so the 16 lanes of
// every group land on 16 distinct 16-B slots of the 256-B bank line.
#include "common.h"
#include <stdexcept>

namespace rdb {

namespace {

typedef int i32x8 __attribute__((ext_vector_type(8)));
typedef __attribute__((address_space(3))) void* lds_ptr_t;

constexpr uint32_t kOOB = 0x80000000u;   // voffset beyond every num_records: the load returns 0
constexpr int kBK = 128;                 // bytes (= e4m3 elements) of K per step

__device__ __forceinline__ __amdgpu_buffer_rsrc_t make_rsrc(const void* p, uint32_t bytes) {
  const uint64_t a = reinterpret_cast<uint64_t>(p);
  const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)a);
  const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)(a >> 32));
  void* base = reinterpret_cast<void*>(((uint64_t)hi << 32) | lo);
  return __builtin_amdgcn_make_buffer_rsrc(base, (short)0, (int)__builtin_amdgcn_readfirstlane(bytes), 0x00020000);
}
__device__ __forceinline__ void dma16(__amdgpu_buffer_rsrc_t r, char* lds, uint32_t off) {
  __builtin_amdgcn_raw_ptr_buffer_load_lds(r, (lds_ptr_t)lds, 16, off, 0, 0, 0);
}

// row pair p = (row >> 1) & 7: p in {2,3,4,5} -> keys {0,2,4,6}, p in {6,7,0,1} -> {1,3,5,7}
__device__ __forceinline__ int swz_key(int row) {
  const int q = ((row >> 1) + 2) & 7;
  return ((q & 3) << 1) | ((q >> 2) ^ 1);
}

// The one MFMA step: D += A(16 x 128) . B(128 x 16), e4m3 x e4m3 (format
// selectors cbsz = blgp = 0), every E8M0 scale byte 127 = 1.0.  Lane l holds
// row / column l & 15 and the 32 consecutive k bytes 32 * (l >> 4) .. + 31 of
// both operands; D is the standard 16x16 layout (column l & 15, rows
// 4 * (l >> 4) + reg).
__device__ __forceinline__ f32x4 mfma_step(const i32x8& a, const i32x8& b, const f32x4& c) {
  return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a, b, c, 0, 0, 0, 0x7F7F7F7F, 0, 0x7F7F7F7F);
}

template <int AUX>
struct Aux16 { typedef bf16 type; };
template <>
struct Aux16<1> { typedef f16 type; };
template <int OUT>
struct OutOf { typedef bf16 type; };
template <>
struct OutOf<1> { typedef f16 type; };
template <>
struct OutOf<2> { typedef float type; };

template <typename O, int NE>
__device__ __forceinline__ void store_vec(O* p, const float* v) {
  typedef O vec __attribute__((ext_vector_type(NE)));
  vec o;
#pragma unroll
  for (int e = 0; e < NE; ++e) o[e] = (O)v[e];
  *reinterpret_cast<vec*>(p) = o;
}

// BM x BN block tile, 4 waves as WGM x WGN, OUT: 0 bf16 / 1 f16 / 2 f32 output,
// AUX: 0 bf16 / 1 f16 bias and residual.
template <int BM, int BN, int WGM, int WGN, int STAGES, int OUT, int AUX>
__global__ void __launch_bounds__(256)
gemm_fp8_kernel(const uint8_t* __restrict__ A, int lda, const uint8_t* __restrict__ W, int ldw,
                const float* __restrict__ sa, const float* __restrict__ sw, void* __restrict__ Cv, int ldc,
                const void* __restrict__ biasv, const void* __restrict__ Rv, int ldr, int M, int N, int K, int act) {
  typedef typename OutOf<OUT>::type OutT;
  typedef typename Aux16<AUX>::type AuxT;
  static_assert(WGM * WGN == 4 && BM % (16 * WGM) == 0 && BN % (16 * WGN) == 0, "4 waves of 16x16 fragments");
  static_assert(BM % 32 == 0 && BN % 32 == 0, "whole 8-row DMA pieces per wave");
  constexpr int WM = BM / WGM, WN = BN / WGN, TM = WM / 16, TN = WN / 16;
  constexpr int A_P = BM / 32, W_P = BN / 32;          // DMA instructions per wave per stage
  constexpr int kStage = (BM + BN) * kBK;
  __shared__ __attribute__((aligned(16))) char smem[STAGES * kStage];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wid / WGN, wn = wid % WGN;
  const int tiles_n = (N + BN - 1) / BN, tiles_m = (M + BM - 1) / BM;
  const int t = xcd_remap(blockIdx.x, tiles_m * tiles_n);
  const int tile_m = t / tiles_n, tile_n = t - tile_m * tiles_n;
  const int m0 = tile_m * BM, n0 = tile_n * BN;

  // ---- staging: lane l of piece p fills row 8p + l/8, physical chunk l%8, with logical chunk (l%8) ^ key(row)
  const __amdgpu_buffer_rsrc_t asrc = make_rsrc(A, (uint32_t)((size_t)(M - 1) * lda + K));
  const __amdgpu_buffer_rsrc_t wsrc = make_rsrc(W, (uint32_t)((size_t)(N - 1) * ldw + K));
  uint32_t aoff[A_P], woff[W_P];
#pragma unroll
  for (int i = 0; i < A_P; ++i) {
    const int row = (wid * A_P + i) * 8 + (lane >> 3);
    const int gm = m0 + row;
    aoff[i] = gm < M ? (uint32_t)((size_t)gm * lda + (((lane & 7) ^ swz_key(row)) << 4)) : kOOB;
  }
#pragma unroll
  for (int i = 0; i < W_P; ++i) {
    const int row = (wid * W_P + i) * 8 + (lane >> 3);
    const int gn = n0 + row;
    woff[i] = gn < N ? (uint32_t)((size_t)gn * ldw + (((lane & 7) ^ swz_key(row)) << 4)) : kOOB;
  }
  auto stage = [&](int buf, int k0) {
    char* base = smem + buf * kStage;
#pragma unroll
    for (int i = 0; i < A_P; ++i) dma16(asrc, base + (wid * A_P + i) * 1024, aoff[i] == kOOB ? kOOB : aoff[i] + k0);
#pragma unroll
    for (int i = 0; i < W_P; ++i)
      dma16(wsrc, base + BM * kBK + (wid * W_P + i) * 1024, woff[i] == kOOB ? kOOB : woff[i] + k0);
  };

  f32x4 acc[TN][TM];
#pragma unroll
  for (int i = 0; i < TN; ++i)
#pragma unroll
    for (int j = 0; j < TM; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  // ---- fragment reads: fragment rows start at multiples of 16, so the key depends on fr only
  const int fr = lane & 15, fg = lane >> 4;
  const int key = swz_key(fr);
  const int foff0 = fr * kBK + (((2 * fg) ^ key) << 4), foff1 = fr * kBK + (((2 * fg + 1) ^ key) << 4);
  auto frag = [&](const char* rows16) {
    const u32x4 lo = *reinterpret_cast<const u32x4*>(rows16 + foff0);
    const u32x4 hi = *reinterpret_cast<const u32x4*>(rows16 + foff1);
    return i32x8{(int)lo[0], (int)lo[1], (int)lo[2], (int)lo[3], (int)hi[0], (int)hi[1], (int)hi[2], (int)hi[3]};
  };
  auto compute = [&](int buf) {
    const char* pa = smem + buf * kStage + wm * WM * kBK;
    const char* pw = smem + buf * kStage + BM * kBK + wn * WN * kBK;
    i32x8 wf[TN], af[TM];
#pragma unroll
    for (int i = 0; i < TN; ++i) wf[i] = frag(pw + i * 16 * kBK);
#pragma unroll
    for (int j = 0; j < TM; ++j) af[j] = frag(pa + j * 16 * kBK);
    // W is the MFMA's A operand: a lane then holds C[m = fr][n = 4 * fg .. + 3], 4 consecutive outputs
#pragma unroll
    for (int i = 0; i < TN; ++i)
#pragma unroll
      for (int j = 0; j < TM; ++j) acc[i][j] = mfma_step(wf[i], af[j], acc[i][j]);
  };

  // ---- main loop: STAGES - 1 tiles in flight; each wave retires its own DMA of
  // tile k (counted vmcnt), the raw barrier publishes every wave's pieces and
  // orders compute(k - 1)'s reads before that buffer is refilled
  const int nk = K / kBK;
  constexpr int kPend = (A_P + W_P) * (STAGES - 2);
  static_assert(kPend < 64, "vmcnt field is 6 bits");
  constexpr int kWaitPend = (kPend & 15) | ((kPend >> 4) << 14) | 0x70 | 0xF00;   // vmcnt(kPend)
  constexpr int kWaitAll = 0x70 | 0xF00;                                           // vmcnt(0)
#pragma unroll
  for (int p = 0; p < STAGES - 1; ++p)
    if (p < nk) stage(p, p * kBK);
  int buf = 0;
  for (int kt = 0; kt < nk; ++kt) {
    if (kt + STAGES - 2 < nk) __builtin_amdgcn_s_waitcnt(kWaitPend);
    else __builtin_amdgcn_s_waitcnt(kWaitAll);
    asm volatile("" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    if (kt + STAGES - 1 < nk) stage(buf == 0 ? STAGES - 1 : buf - 1, (kt + STAGES - 1) * kBK);
    compute(buf);
    buf = buf == STAGES - 1 ? 0 : buf + 1;
  }

  // ---- epilogue: lane holds C[m][n .. n + 3]; N % 8 == 0, so n < N covers the four
  OutT* C = static_cast<OutT*>(Cv);
  const AuxT* bias = static_cast<const AuxT*>(biasv);
  const AuxT* R = static_cast<const AuxT*>(Rv);
  const bool swiglu = act == ACT_SWIGLU;
  auto run = [&](auto actf) {
#pragma unroll
    for (int i = 0; i < TN; ++i) {
      const int n = n0 + wn * WN + i * 16 + fg * 4;
      if (n >= N) continue;
      const f32x4 s4 = *reinterpret_cast<const f32x4*>(sw + n);
      float b[4] = {0.f, 0.f, 0.f, 0.f};
      if (bias != nullptr) {
        const u32x2 raw = *reinterpret_cast<const u32x2*>(bias + n);
        const AuxT* e = reinterpret_cast<const AuxT*>(&raw);
#pragma unroll
        for (int q = 0; q < 4; ++q) b[q] = (float)e[q];
      }
#pragma unroll
      for (int j = 0; j < TM; ++j) {
        const int m = m0 + wm * WM + j * 16 + fr;
        if (m >= M) continue;
        const float am = sa[m];
        float x[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) x[q] = acc[i][j][q] * am * s4[q] + b[q];
        if (swiglu) {
          float o[2] = {apply_act<ACT_SILU>(x[0]) * x[1], apply_act<ACT_SILU>(x[2]) * x[3]};
          const size_t at = (size_t)m * ldr + (n >> 1);
          if (R != nullptr) {
            const uint32_t raw = *reinterpret_cast<const uint32_t*>(R + at);
            const AuxT* e = reinterpret_cast<const AuxT*>(&raw);
            o[0] += (float)e[0];
            o[1] += (float)e[1];
          }
          store_vec<OutT, 2>(C + (size_t)m * ldc + (n >> 1), o);
        } else {
#pragma unroll
          for (int q = 0; q < 4; ++q) x[q] = actf(x[q]);
          if (R != nullptr) {
            const u32x2 raw = *reinterpret_cast<const u32x2*>(R + (size_t)m * ldr + n);
            const AuxT* e = reinterpret_cast<const AuxT*>(&raw);
#pragma unroll
            for (int q = 0; q < 4; ++q) x[q] += (float)e[q];
          }
          store_vec<OutT, 4>(C + (size_t)m * ldc + n, x);
        }
      }
    }
  };
  switch (act) {
    case ACT_GELU: run([](float x) { return apply_act<ACT_GELU>(x); }); break;
    case ACT_SILU: run([](float x) { return apply_act<ACT_SILU>(x); }); break;
    default: run([](float x) { return x; }); break;
  }
}

struct Fp8Tile { int bm, bn; };
// 0, 1: grids that fill the GPU; 2, 3: small M (the Llama projections at M = 128 .. 512).
// A 64 x 128 tile was measured too and never led (bench/fp8_probe.py).
constexpr Fp8Tile kFp8Tiles[] = {{128, 256}, {128, 128}, {64, 64}, {32, 64}};
// The static rule: the first tile whose grid has between these many blocks (256 CUs).
// Thresholds from bench/fp8_probe.py at M = 128 .. 1024 (profiles/fp8_llama_r7.json):
// 128 x 256 halves the staged bytes per FLOP again but runs one block per CU, so it
// leads only while its grid is one to two rounds of the CUs.
constexpr int kFp8MinBlocks[] = {192, 192, 160, 0};
constexpr int kFp8MaxBlocks[] = {512, 1 << 30, 1 << 30, 1 << 30};
constexpr int kFp8NumTiles = sizeof(kFp8Tiles) / sizeof(kFp8Tiles[0]);

template <int BM, int BN, int WGM, int WGN, int STAGES>
void launch_tile(int out_dtype, int aux_dtype, hipStream_t s, const uint8_t* A, int lda, const uint8_t* W, int ldw,
                 const float* sa, const float* sw, void* C, int ldc, const void* bias, const void* R, int ldr, int M,
                 int N, int K, int act) {
  const dim3 grid(((M + BM - 1) / BM) * ((N + BN - 1) / BN)), blk(256);
#define RDB_F8_GO(OUT, AUX)                                                                                     \
  hipLaunchKernelGGL((gemm_fp8_kernel<BM, BN, WGM, WGN, STAGES, OUT, AUX>), grid, blk, 0, s, A, lda, W, ldw, sa, \
                     sw, C, ldc, bias, R, ldr, M, N, K, act)
  if (out_dtype == 0) RDB_F8_GO(0, 0);
  else if (out_dtype == 1) RDB_F8_GO(1, 1);
  else if (aux_dtype == 1) RDB_F8_GO(2, 1);
  else RDB_F8_GO(2, 0);
#undef RDB_F8_GO
}

}  // namespace

int gemm_fp8_num_tiles() { return kFp8NumTiles; }

// tile < 0: the static rule above; the smallest tile when no grid is large enough
int gemm_fp8_pick_tile(int M, int N) {
  for (int c = 0; c < kFp8NumTiles; ++c) {
    const long blocks = (long)((M + kFp8Tiles[c].bm - 1) / kFp8Tiles[c].bm) * ((N + kFp8Tiles[c].bn - 1) / kFp8Tiles[c].bn);
    if (blocks >= kFp8MinBlocks[c] && blocks <= kFp8MaxBlocks[c]) return c;
  }
  return kFp8NumTiles - 1;
}

void gemm_fp8(int out_dtype, int aux_dtype, uintptr_t A, int lda, uintptr_t W, int ldw, uintptr_t sa, uintptr_t sw,
              uintptr_t C, int ldc, uintptr_t bias, uintptr_t R, int ldr, int M, int N, int K, int act, int tile,
              uintptr_t stream) {
  if (M < 1 || N < 8 || N % 8 != 0 || K < kBK || K % kBK != 0)
    throw std::invalid_argument("gemm_fp8: need M >= 1, N % 8 == 0, K % 128 == 0");
  if (act != ACT_NONE && act != ACT_GELU && act != ACT_SILU && act != ACT_SWIGLU)
    throw std::invalid_argument("gemm_fp8: act must be none, gelu, silu or swiglu");
  if (out_dtype < 0 || out_dtype > 2 || aux_dtype < 0 || aux_dtype > 1 || (out_dtype < 2 && aux_dtype != out_dtype))
    throw std::invalid_argument("gemm_fp8: bad output / bias dtype");
  const int n_out = act == ACT_SWIGLU ? N / 2 : N;
  if (lda < K || ldw < K || lda % 16 != 0 || ldw % 16 != 0 || ((A | W | sa | sw | C | bias | R) & 15) ||
      ldc != n_out || (R != 0 && ldr != n_out))
    throw std::invalid_argument("gemm_fp8: bad strides or alignment");
  if ((size_t)M * lda >= (1ull << 31) || (size_t)N * ldw >= (1ull << 31))
    throw std::invalid_argument("gemm_fp8: operand larger than 2 GiB");
  if (tile < 0) tile = gemm_fp8_pick_tile(M, N);
  if (tile >= kFp8NumTiles) throw std::invalid_argument("gemm_fp8: no such tile");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
#define RDB_F8_ARGS out_dtype, aux_dtype, s, (const uint8_t*)A, lda, (const uint8_t*)W, ldw, (const float*)sa, \
                    (const float*)sw, (void*)C, ldc, (const void*)bias, (const void*)R, ldr, M, N, K, act
  if (tile == 0) launch_tile<128, 256, 2, 2, 3>(RDB_F8_ARGS);
  else if (tile == 1) launch_tile<128, 128, 2, 2, 3>(RDB_F8_ARGS);
  else if (tile == 2) launch_tile<64, 64, 2, 2, 4>(RDB_F8_ARGS);
  else launch_tile<32, 64, 1, 4, 4>(RDB_F8_ARGS);
#undef RDB_F8_ARGS
  RDB_HIP_CHECK(hipGetLastError());
}

}  // namespace rdb
