// Backward-pass kernels of PredictionHead and its ResNets (resnet.py, rf.py:1130-1172), of the pair axial attention, of
// OuterProductMean (rf_layernorm_bwd_fused) and of GraphTransformer and its block (end of file) on gfx950: the weight gradient of a
// stride-1 "same" convolution (pixel contraction), InstanceNorm2d(affine) backward, LayerNorm backward, and the absolute
// maximum the fp16 build scales its gradients by.  Input gradients of the convolutions / Linears run on rf_gemm (the forward's
// implicit-GEMM engine with a repacked weight); these kernels are what the forward does not already have.
// Every reduction writes per-block partials to a caller-owned workspace and adds them in a fixed order: no atomics, results
// are bitwise reproducible run to run (like rf_instnorm_stats).
#include "common.h"

#define RF_CHECK_DT(dt) \
  if ((dt) != RF_F32 && (dt) != RF_H16) return RF_EINVAL

static inline unsigned cdiv(int64_t a, int64_t b) { return (unsigned)((a + b - 1) / b); }

typedef __attribute__((ext_vector_type(4))) short s16x4;
typedef __attribute__((address_space(3))) s16x4 lds_s16x4;

// ================================================================================================
// rf_conv_wgrad:  dW[co][tap][ci] = alpha * sum_{b,p} dY[b,p,co] * X[b, p + delta(tap), ci]   (zero outside the picture)
// ================================================================================================
#define WG_KP 32           // pixels per k-step: the K of one v_mfma_f32_16x16x32
#define WG_TARGET_WGS 1024 // workgroups to aim for: the pixel axis is split until (tiles x splits) reaches this
#define WG32_PIX 64        // fp32 kernel: pixels per split unit

// pixel split shared by the host-side size query and the launch: depends on the shape only (never on the device)
static void wgrad_split(int dtype, int64_t P, int Co, int Ci, int taps, int* tiles, int* splits, int64_t* unit_per_split) {
  int64_t units, t;
  if (dtype == RF_F32) {
    t = (int64_t)cdiv(Ci, 64) * cdiv(Co, 16);
    units = cdiv(P, WG32_PIX);
  } else {
    const bool tall = taps == 9 && Co % 96 == 0;  // 96 x 32 tiles (3 waves) cover C = 288 without padding
    t = tall ? (int64_t)(Co / 96) * cdiv(Ci, 32) : (int64_t)cdiv(Co, 64) * cdiv(Ci, 64);
    units = cdiv(P, WG_KP);
  }
  int64_t s = (WG_TARGET_WGS + t - 1) / t;
  if (s > units) s = units;
  if (s < 1) s = 1;
  const int64_t ups = (units + s - 1) / s;
  s = (units + ups - 1) / ups;  // no empty split
  *tiles = (int)t;
  *splits = (int)s;
  *unit_per_split = ups;
}

// 16-bit operands, fp32 accumulation.  Workgroup = WM x WN waves, each wave a 32(co) x 32(ci) tile for all TAPS taps.  Per
// 32-pixel k-step the dY tile [32 px][CO_T] and the TAPS shifted X windows [32 px][CI_T] are staged into LDS with 16-byte
// loads (zero outside the picture, past the split's last pixel and past Co / Ci: the tiles are padded, never masked) and read
// as MFMA operands with ds_read_b64_tr_b16: both operands contract over the pixel (row) index of a [pixel][channel] image.
template <int TAPS, int WM, int WN>
__global__ __launch_bounds__(64 * WM * WN) void conv_wgrad_h16_kernel(const h16_t* __restrict__ dy, const h16_t* __restrict__ x,
                                                                   float* __restrict__ ws, float* __restrict__ bws, int H,
                                                                   int W, int64_t P, int Co, int Ci, int dil, int ci_tiles,
                                                                   int64_t ups) {
  constexpr int NT = 64 * WM * WN;
  constexpr int CO_T = 32 * WM, CI_T = 32 * WN;
  constexpr int DP = CO_T + 8, XP = CI_T + 8;  // row pitches (elements): +16 bytes, rows stay 8-byte aligned
  __shared__ __attribute__((aligned(16))) h16_t sdy[WG_KP * DP];
  __shared__ __attribute__((aligned(16))) h16_t sx[TAPS * WG_KP * XP];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave % WM, wn = wave / WM;
  const int co0 = (blockIdx.x / ci_tiles) * CO_T, ci0 = (blockIdx.x % ci_tiles) * CI_T;
  const int split = blockIdx.y;
  const int64_t p_begin = (int64_t)split * ups * WG_KP;
  int64_t p_end = p_begin + ups * WG_KP;
  if (p_end > P) p_end = P;
  const int64_t HW = (int64_t)H * W;
  const bool do_bias = bws != nullptr && ci0 == 0;

  f32x4 acc[TAPS][2][2];
#pragma unroll
  for (int t = 0; t < TAPS; ++t)
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int b = 0; b < 2; ++b) acc[t][a][b] = (f32x4){0.f, 0.f, 0.f, 0.f};
  float bsum = 0.f;  // thread tid < CO_T: bias partial of channel co0 + tid

  // ds_read_b64_tr_b16 addressing (cdna_hip_programming T10): lane 4q+p of a 16-lane group g supplies row 8g + 4h + q,
  // columns 4p..4p+3 of the 16-column block; it receives column (lane & 15) of those 4 rows, i.e. k = 8g + 4h + 0..3
  const int g = lane >> 4, q = (lane & 15) >> 2, pcol = (lane & 3) * 4;

  for (int64_t pc = p_begin; pc < p_end; pc += WG_KP) {
    // ---- stage dY[pc .. pc+31][co0 .. co0+CO_T) ----
    for (int v = tid; v < WG_KP * (CO_T / 8); v += NT) {
      const int px = v / (CO_T / 8), cv = (v % (CO_T / 8)) * 8;
      const int64_t p = pc + px;
      h16x8 val = (h16x8){0, 0, 0, 0, 0, 0, 0, 0};
      if (p < p_end && co0 + cv < Co) val = *(const h16x8*)(dy + p * Co + co0 + cv);
      *(h16x8*)(sdy + px * DP + cv) = val;
    }
    // ---- stage the TAPS shifted windows of X ----
    for (int v = tid; v < TAPS * WG_KP * (CI_T / 8); v += NT) {
      const int t = v / (WG_KP * (CI_T / 8));
      const int r = v % (WG_KP * (CI_T / 8));
      const int px = r / (CI_T / 8), cv = (r % (CI_T / 8)) * 8;
      const int64_t p = pc + px;
      h16x8 val = (h16x8){0, 0, 0, 0, 0, 0, 0, 0};
      if (p < p_end && ci0 + cv < Ci) {
        const int64_t bb = p / HW, rr = p % HW;
        const int i = (int)(rr / W) + (TAPS == 9 ? (t / 3 - 1) * dil : 0);
        const int j = (int)(rr % W) + (TAPS == 9 ? (t % 3 - 1) * dil : 0);
        if (i >= 0 && i < H && j >= 0 && j < W) val = *(const h16x8*)(x + ((bb * H + i) * W + j) * Ci + ci0 + cv);
      }
      *(h16x8*)(sx + (t * WG_KP + px) * XP + cv) = val;
    }
    __syncthreads();
    if (do_bias && tid < CO_T) {
#pragma unroll 8
      for (int px = 0; px < WG_KP; ++px) bsum += h2f(sdy[px * DP + tid]);
    }
    // ---- MFMA: every lane of every wave takes part (EXEC all ones for the transposed reads) ----
    h16x8 af[2];
#pragma unroll
    for (int a = 0; a < 2; ++a) {
      const int col = wm * 32 + a * 16 + pcol;
      const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(sdy + (8 * g + q) * DP + col));
      const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(sdy + (8 * g + 4 + q) * DP + col));
      af[a] = (h16x8){lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    }
#pragma unroll
    for (int t = 0; t < TAPS; ++t) {
      h16x8 bf[2];
#pragma unroll
      for (int b = 0; b < 2; ++b) {
        const int col = wn * 32 + b * 16 + pcol;
        const h16_t* base = sx + t * WG_KP * XP;
        const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(base + (8 * g + q) * XP + col));
        const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(base + (8 * g + 4 + q) * XP + col));
        bf[b] = (h16x8){lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
      }
#pragma unroll
      for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) acc[t][a][b] = rf_mfma16(af[a], bf[b], acc[t][a][b], 0, 0, 0);
    }
    __syncthreads();
  }
  // ---- partials: ws[split][co][tap][ci]; D layout of 16x16: col = lane & 15 (ci), row = 4 (lane >> 4) + r (co) ----
  float* wsp = ws + (int64_t)split * Co * TAPS * Ci;
#pragma unroll
  for (int t = 0; t < TAPS; ++t)
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int b = 0; b < 2; ++b) {
        const int ci = ci0 + wn * 32 + b * 16 + (lane & 15);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int co = co0 + wm * 32 + a * 16 + 4 * (lane >> 4) + r;
          if (co < Co && ci < Ci) wsp[((int64_t)co * TAPS + t) * Ci + ci] = acc[t][a][b][r];
        }
      }
  if (do_bias && tid < CO_T && co0 + tid < Co) bws[(int64_t)split * Co + co0 + tid] = bsum;
}

// exact fp32: thread (ci = ci0 + tid % 64, co = co0 + 4 (tid / 64) + 0..3) accumulates all taps over its split's pixels
template <int TAPS>
__global__ __launch_bounds__(256) void conv_wgrad_f32_kernel(const float* __restrict__ dy, const float* __restrict__ x,
                                                              float* __restrict__ ws, float* __restrict__ bws, int H, int W,
                                                              int64_t P, int Co, int Ci, int dil, int64_t ups) {
  const int ci = blockIdx.x * 64 + (threadIdx.x & 63);
  const int co_b = blockIdx.y * 16 + (threadIdx.x >> 6) * 4;
  const int split = blockIdx.z;
  const int64_t p_begin = (int64_t)split * ups * WG32_PIX;
  int64_t p_end = p_begin + ups * WG32_PIX;
  if (p_end > P) p_end = P;
  const int64_t HW = (int64_t)H * W;
  float acc[TAPS][4], bs[4];
#pragma unroll
  for (int t = 0; t < TAPS; ++t)
#pragma unroll
    for (int u = 0; u < 4; ++u) acc[t][u] = 0.f;
#pragma unroll
  for (int u = 0; u < 4; ++u) bs[u] = 0.f;
  const bool ci_ok = ci < Ci;
  for (int64_t p = p_begin; p < p_end; ++p) {
    float d[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) d[u] = co_b + u < Co ? dy[p * Co + co_b + u] : 0.f;
#pragma unroll
    for (int u = 0; u < 4; ++u) bs[u] += d[u];
    const int64_t bb = p / HW, rr = p % HW;
    const int i0 = (int)(rr / W), j0 = (int)(rr % W);
#pragma unroll
    for (int t = 0; t < TAPS; ++t) {
      const int i = i0 + (TAPS == 9 ? (t / 3 - 1) * dil : 0), j = j0 + (TAPS == 9 ? (t % 3 - 1) * dil : 0);
      const float xv = ci_ok && i >= 0 && i < H && j >= 0 && j < W ? x[((bb * H + i) * W + j) * Ci + ci] : 0.f;
#pragma unroll
      for (int u = 0; u < 4; ++u) acc[t][u] = fmaf(d[u], xv, acc[t][u]);
    }
  }
  float* wsp = ws + (int64_t)split * Co * TAPS * Ci;
  if (ci_ok)
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (co_b + u < Co)
#pragma unroll
        for (int t = 0; t < TAPS; ++t) wsp[((int64_t)(co_b + u) * TAPS + t) * Ci + ci] = acc[t][u];
  if (bws && blockIdx.x == 0 && (threadIdx.x & 63) == 0)
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (co_b + u < Co) bws[(int64_t)split * Co + co_b + u] = bs[u];
}

// out[e] = alpha * sum_{s = 0 .. S-1} part[s][e], in split order
__global__ __launch_bounds__(256) void ordered_split_sum_kernel(const float* __restrict__ part, float* __restrict__ out, int64_t n,
                                                                int S, float alpha) {
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (int64_t)gridDim.x * 256) {
    float s = 0.f;
    for (int k = 0; k < S; ++k) s += part[(int64_t)k * n + e];
    out[e] = alpha * s;
  }
}

extern "C" int64_t rf_conv_wgrad_ws_bytes(int dtype, int B, int H, int W, int Co, int Ci, int taps) {
  if (B <= 0 || H <= 0 || W <= 0 || Co <= 0 || Ci <= 0 || (taps != 1 && taps != 9)) return 0;
  int tiles, S;
  int64_t ups;
  wgrad_split(dtype, (int64_t)B * H * W, Co, Ci, taps, &tiles, &S, &ups);
  return (int64_t)S * ((int64_t)Co * taps * Ci + Co) * (int64_t)sizeof(float);
}

extern "C" int rf_conv_wgrad(const void* dy, const void* x, int dtype, float* dw, float* dbias, int B, int H, int W, int Co,
                             int Ci, int taps, int dilation, float alpha, void* workspace, int64_t ws_bytes, void* stream) {
  RF_CHECK_DT(dtype);
  if (!dy || !x || !dw || B <= 0 || H <= 0 || W <= 0 || Co <= 0 || Ci <= 0) return RF_EINVAL;
  if (taps != 1 && taps != 9) return RF_EINVAL;
  if (taps == 9 && (dilation < 1 || dilation > 8)) return RF_EINVAL;
  if (!workspace || ws_bytes < rf_conv_wgrad_ws_bytes(dtype, B, H, W, Co, Ci, taps)) return RF_EINVAL;
  const int64_t P = (int64_t)B * H * W;
  int tiles, S;
  int64_t ups;
  wgrad_split(dtype, P, Co, Ci, taps, &tiles, &S, &ups);
  float* ws = (float*)workspace;
  float* bws = dbias ? ws + (int64_t)S * Co * taps * Ci : nullptr;
  hipStream_t s = (hipStream_t)stream;
  const int dil = taps == 9 ? dilation : 1;
  if (dtype == RF_F32) {
    if (((uintptr_t)dy % 4) || ((uintptr_t)x % 4)) return RF_EALIGN;
    dim3 grid(cdiv(Ci, 64), cdiv(Co, 16), S);
    if (taps == 9)
      hipLaunchKernelGGL(conv_wgrad_f32_kernel<9>, grid, dim3(256), 0, s, (const float*)dy, (const float*)x, ws, bws, H, W, P, Co,
                         Ci, dil, ups);
    else
      hipLaunchKernelGGL(conv_wgrad_f32_kernel<1>, grid, dim3(256), 0, s, (const float*)dy, (const float*)x, ws, bws, H, W, P, Co,
                         Ci, dil, ups);
  } else {
    // 16-byte channel vectors: rows of 8-channel multiples, 16-byte aligned bases
    if (Co % 8 || Ci % 8 || ((uintptr_t)dy % 16) || ((uintptr_t)x % 16)) return RF_EALIGN;
    const h16_t* d16 = (const h16_t*)dy;
    const h16_t* x16 = (const h16_t*)x;
    if (taps == 9 && Co % 96 == 0) {
      const int cit = (int)cdiv(Ci, 32);
      hipLaunchKernelGGL((conv_wgrad_h16_kernel<9, 3, 1>), dim3((Co / 96) * cit, S), dim3(192), 0, s, d16, x16, ws, bws, H, W,
                         P, Co, Ci, dil, cit, ups);
    } else {
      const int cit = (int)cdiv(Ci, 64);
      const dim3 grid(cdiv(Co, 64) * cit, S);
      if (taps == 9)
        hipLaunchKernelGGL((conv_wgrad_h16_kernel<9, 2, 2>), grid, dim3(256), 0, s, d16, x16, ws, bws, H, W, P, Co, Ci, dil,
                           cit, ups);
      else
        hipLaunchKernelGGL((conv_wgrad_h16_kernel<1, 2, 2>), grid, dim3(256), 0, s, d16, x16, ws, bws, H, W, P, Co, Ci, dil,
                           cit, ups);
    }
  }
  const int64_t n = (int64_t)Co * taps * Ci;
  hipLaunchKernelGGL(ordered_split_sum_kernel, dim3(min(cdiv(n, 256), 4096u)), dim3(256), 0, s, ws, dw, n, S, alpha);
  if (dbias)
    hipLaunchKernelGGL(ordered_split_sum_kernel, dim3(cdiv(Co, 256)), dim3(256), 0, s, bws, dbias, (int64_t)Co, S, alpha);
  return rf_launch_status();
}

// ================================================================================================
// rf_instnorm_bwd
// ================================================================================================
#define INB_PIX 128  // pixels per statistics block: the partials have the shape of rf_instnorm_stats' (rf_instnorm_ws_bytes)

__device__ __forceinline__ void in_stats(const double* sums, int64_t i, int64_t HW, float eps, float* mean, float* rstd) {
  const double s = sums[i * 2], q = sums[i * 2 + 1];
  const double m = s / (double)HW;
  double var = q / (double)HW - m * m;
  var = var > 0.0 ? var : 0.0;
  *mean = (float)m;
  *rstd = rsqrtf((float)var + eps);
}

// incoming gradient times the ELU derivative taken from the ELU output a (y > 0 ? 1 : y + 1)
__device__ __forceinline__ float in_geff(const float* g, const void* a, int a_dt, int64_t e) {
  float v = g[e];
  if (a) {
    const float y = ld(a, a_dt, e);
    v *= y > 0.f ? 1.f : y + 1.f;
  }
  return v;
}

__global__ __launch_bounds__(256) void instnorm_bwd_stats_kernel(const float* g, const void* a, int a_dt, const void* x, int x_dt,
                                                                 const double* sums, float eps, float* partials, int64_t HW,
                                                                 int C) {
  const int b = blockIdx.y;
  const int64_t p0 = (int64_t)blockIdx.x * INB_PIX;
  const int64_t p1 = p0 + INB_PIX < HW ? p0 + INB_PIX : HW;
  for (int c = threadIdx.x; c < C; c += 256) {
    float mean, rstd;
    in_stats(sums, (int64_t)b * C + c, HW, eps, &mean, &rstd);
    float sg = 0.f, sgx = 0.f;
    for (int64_t p = p0; p < p1; ++p) {
      const int64_t e = ((int64_t)b * HW + p) * C + c;
      const float ge = in_geff(g, a, a_dt, e);
      sg += ge;
      sgx = fmaf(ge, (ld(x, x_dt, e) - mean) * rstd, sgx);
    }
    float* pp = partials + ((int64_t)b * gridDim.x + blockIdx.x) * 2 * C;
    pp[c] = sg;
    pp[C + c] = sgx;
  }
}

// per (b, c): (sum g, sum g xhat) in block order (fp64) -> coef[b][c] = (mean, rstd, mean g, mean g xhat) for the apply pass;
// dbeta[c] / dgamma[c] = the sums over b in sample order
__global__ __launch_bounds__(256) void instnorm_bwd_finalize_kernel(const float* partials, const double* sums, float eps,
                                                                    float4* coef, float* dgamma, float* dbeta, int B, int nblk,
                                                                    int64_t HW, int C) {
  for (int c = blockIdx.x * 256 + threadIdx.x; c < C; c += gridDim.x * 256) {
    double tg = 0.0, tx = 0.0;
    for (int b = 0; b < B; ++b) {
      double sg = 0.0, sx = 0.0;
      for (int k = 0; k < nblk; ++k) {
        const float* pp = partials + ((int64_t)b * nblk + k) * 2 * C;
        sg += (double)pp[c];
        sx += (double)pp[C + c];
      }
      float mean, rstd;
      in_stats(sums, (int64_t)b * C + c, HW, eps, &mean, &rstd);
      coef[(int64_t)b * C + c] = make_float4(mean, rstd, (float)(sg / (double)HW), (float)(sx / (double)HW));
      tg += sg;
      tx += sx;
    }
    if (dbeta) dbeta[c] = (float)tg;
    if (dgamma) dgamma[c] = (float)tx;
  }
}

// dx = gamma / sigma * (g - mean g - xhat * mean(g xhat))
__global__ __launch_bounds__(256) void instnorm_bwd_apply_kernel(const float* g, const void* a, int a_dt, const void* x, int x_dt,
                                                                 const float4* coef, const float* gamma, void* dx, int dx_dt,
                                                                 float* ge_out, int64_t HW, int C, int64_t total) {
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
    const int c = (int)(e % C);
    const float4 k = coef[(e / (HW * C)) * C + c];
    const float xh = (ld(x, x_dt, e) - k.x) * k.y;
    const float ge = in_geff(g, a, a_dt, e);
    st(dx, dx_dt, e, gamma[c] * k.y * (ge - k.z - xh * k.w));
    if (ge_out) ge_out[e] = ge;  // (may alias g: each element is read and written by the same thread)
  }
}

extern "C" int rf_instnorm_bwd(const float* g, const void* act_out, int act_dtype, const void* x, int x_dtype, const void* sums,
                               const float* gamma, float eps, void* dx, int dx_dtype, float* ge_out, float* dgamma, float* dbeta,
                               int B, int64_t HW, int C, void* workspace, int64_t ws_bytes, void* stream) {
  RF_CHECK_DT(x_dtype);
  RF_CHECK_DT(dx_dtype);
  if (act_out) RF_CHECK_DT(act_dtype);
  if (!g || !x || !sums || !gamma || !dx || B <= 0 || HW <= 0 || C <= 0) return RF_EINVAL;
  const unsigned nblk = cdiv(HW, INB_PIX);
  const int64_t part_bytes = (int64_t)B * nblk * 2 * C * (int64_t)sizeof(float);
  const int64_t coef_off = (part_bytes + 15) / 16 * 16;
  if (!workspace || ws_bytes < coef_off + (int64_t)B * C * (int64_t)sizeof(float4) || ((uintptr_t)workspace % 16))
    return RF_EINVAL;
  float* partials = (float*)workspace;
  float4* coef = (float4*)((char*)workspace + coef_off);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(instnorm_bwd_stats_kernel, dim3(nblk, B), dim3(256), 0, s, g, act_out, act_dtype, x, x_dtype,
                     (const double*)sums, eps, partials, HW, C);
  hipLaunchKernelGGL(instnorm_bwd_finalize_kernel, dim3(cdiv(C, 256)), dim3(256), 0, s, partials, (const double*)sums, eps, coef, dgamma,
                     dbeta, B, (int)nblk, HW, C);
  const int64_t total = (int64_t)B * HW * C;
  hipLaunchKernelGGL(instnorm_bwd_apply_kernel, dim3(min(cdiv(total, 256), 16384u)), dim3(256), 0, s, g, act_out, act_dtype, x,
                     x_dtype, (const float4*)coef, gamma, dx, dx_dtype, ge_out, HW, C, total);
  return rf_launch_status();
}

// ================================================================================================
// rf_layernorm_bwd: one wave per row (fp32 statistics recomputed from x), per-block column partials for dgamma / dbeta
// ================================================================================================
#define LNB_ROWS 64     // rows per block (4 waves x 16 rows)
#define LNB_MAXC 16     // D <= 64 * LNB_MAXC

__global__ __launch_bounds__(256) void layernorm_bwd_kernel(const float* x, const float* g, const float* gamma, float eps,
                                                            void* dx, int dx_dt, float* partials, int64_t rows, int D) {
  __shared__ float red[4][2][64 * LNB_MAXC];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int nper = (D + 63) / 64;
  float pg[LNB_MAXC], pgx[LNB_MAXC];
#pragma unroll
  for (int k = 0; k < LNB_MAXC; ++k) pg[k] = pgx[k] = 0.f;
  const int64_t r0 = (int64_t)blockIdx.x * LNB_ROWS;
  for (int rr = wave; rr < LNB_ROWS; rr += 4) {
    const int64_t r = r0 + rr;
    if (r >= rows) break;  // (wave-uniform)
    const float* xr = x + r * D;
    const float* gr = g + r * D;
    float xv[LNB_MAXC], gv[LNB_MAXC];
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < LNB_MAXC; ++k) {
      const int c = lane + 64 * k;
      xv[k] = k < nper && c < D ? xr[c] : 0.f;
      gv[k] = k < nper && c < D ? gr[c] : 0.f;
      s += xv[k];
    }
    const float mean = wave_sum(s) / (float)D;
    float q = 0.f;
#pragma unroll
    for (int k = 0; k < LNB_MAXC; ++k) {
      const int c = lane + 64 * k;
      const float d = k < nper && c < D ? xv[k] - mean : 0.f;
      q = fmaf(d, d, q);
    }
    const float rstd = rsqrtf(wave_sum(q) / (float)D + eps);
    float m1 = 0.f, m2 = 0.f;
#pragma unroll
    for (int k = 0; k < LNB_MAXC; ++k) {
      const int c = lane + 64 * k;
      if (k < nper && c < D) {
        const float xh = (xv[k] - mean) * rstd;
        const float gg = gv[k] * gamma[c];
        m1 += gg;
        m2 = fmaf(gg, xh, m2);
        pg[k] += gv[k];
        pgx[k] = fmaf(gv[k], xh, pgx[k]);
      }
    }
    m1 = wave_sum(m1) / (float)D;
    m2 = wave_sum(m2) / (float)D;
#pragma unroll
    for (int k = 0; k < LNB_MAXC; ++k) {
      const int c = lane + 64 * k;
      if (k < nper && c < D) {
        const float xh = (xv[k] - mean) * rstd;
        st(dx, dx_dt, r * D + c, rstd * (gv[k] * gamma[c] - m1 - xh * m2));
      }
    }
  }
#pragma unroll
  for (int k = 0; k < LNB_MAXC; ++k) {
    red[wave][0][lane + 64 * k] = pg[k];
    red[wave][1][lane + 64 * k] = pgx[k];
  }
  __syncthreads();
  for (int c = threadIdx.x; c < D; c += 256) {
    float tg = 0.f, tx = 0.f;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      tg += red[w][0][c];
      tx += red[w][1][c];
    }
    partials[(int64_t)blockIdx.x * 2 * D + c] = tg;
    partials[(int64_t)blockIdx.x * 2 * D + D + c] = tx;
  }
}

// dbeta[c] = sum_k partials[k][0][c], dgamma[c] = sum_k partials[k][1][c], block order, fp64
// (acc: the sum is added to what dgamma / dbeta hold -- one caller-ordered fp32 addition per call)
__global__ __launch_bounds__(256) void layernorm_bwd_finalize_kernel(const float* partials, float* dgamma, float* dbeta, int nblk,
                                                                     int D, int acc) {
  for (int c = blockIdx.x * 256 + threadIdx.x; c < 2 * D; c += gridDim.x * 256) {
    double t = 0.0;
    for (int k = 0; k < nblk; ++k) t += (double)partials[(int64_t)k * 2 * D + c];
    if (c < D) {
      if (dbeta) dbeta[c] = acc ? dbeta[c] + (float)t : (float)t;
    } else if (dgamma) {
      dgamma[c - D] = acc ? dgamma[c - D] + (float)t : (float)t;
    }
  }
}

extern "C" int64_t rf_layernorm_bwd_ws_bytes(int64_t rows, int D) {
  return (int64_t)cdiv(rows, LNB_ROWS) * 2 * D * (int64_t)sizeof(float);
}

extern "C" int rf_layernorm_bwd(const float* x, const float* g, const float* gamma, float eps, void* dx, int dx_dtype,
                                float* dgamma, float* dbeta, int64_t rows, int D, void* workspace, int64_t ws_bytes,
                                void* stream) {
  RF_CHECK_DT(dx_dtype);
  if (!x || !g || !gamma || !dx || rows <= 0 || D <= 0 || D > 64 * LNB_MAXC) return RF_EINVAL;
  if (!workspace || ws_bytes < rf_layernorm_bwd_ws_bytes(rows, D)) return RF_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  const unsigned nblk = cdiv(rows, LNB_ROWS);
  hipLaunchKernelGGL(layernorm_bwd_kernel, dim3(nblk), dim3(256), 0, s, x, g, gamma, eps, dx, dx_dtype, (float*)workspace, rows,
                     D);
  hipLaunchKernelGGL(layernorm_bwd_finalize_kernel, dim3(cdiv(2 * D, 256)), dim3(256), 0, s, (const float*)workspace, dgamma,
                     dbeta, (int)nblk, D, 0);
  return rf_launch_status();
}

// ================================================================================================
// rf_layernorm_bwd_fused: LayerNorm forward AND backward of a row in one pass over operand-typed rows (OuterProductMean's
// backward, model.py: x = the recomputed outer products, g = W^T dout, both as the GEMMs wrote them).  One wave per row,
// 16-byte loads, the row lives in registers: statistics in fp32 (two-pass, like rf_layernorm), then z = LN(x) and
// dx = rstd * (g gamma - mean(g gamma) - xhat * mean(g gamma xhat)) are written in the operand type, and the wave keeps the
// column sums of g and g xhat of its rows in registers.  Per block they go to partials[block][2][D] (wave order), which
// layernorm_bwd_finalize_kernel adds in block order: no atomics.  Against the chain rf_layernorm -> cast -> cast ->
// rf_layernorm_bwd this reads x and g once instead of three times and never writes an fp32 copy of either.
// dx may alias g and z may alias x: a wave has read its whole row (both reductions depend on it) before it writes.
// ================================================================================================
#define LNF_MAXD 1024

// rows per block: depends on the shape only (the partials' order, hence the result's bits, never on the device)
static int lnf_rows_per_block(int64_t rows) {
  int rpb = 8;
  while (rpb < 64 && rows / rpb > 2048) rpb *= 2;
  return rpb;
}

template <bool H16>
__global__ __launch_bounds__(256) void layernorm_bwd_fused_kernel(const void* x, const void* g, const float* __restrict__ gamma,
                                                                  const float* __restrict__ beta, float eps, void* dx, void* z,
                                                                  float* __restrict__ partials, int64_t rows, int D, int rpb) {
  constexpr int VEC = H16 ? 8 : 4;            // elements of one 16-byte load
  constexpr int NCH = LNF_MAXD / (64 * VEC);  // 16-byte chunks per lane: chunk index = lane + 64 k
  __shared__ float red[4][2][LNF_MAXD];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int nch = D / VEC;
  float gam[NCH][VEC], bet[NCH][VEC], pg[NCH][VEC], pgx[NCH][VEC];
#pragma unroll
  for (int k = 0; k < NCH; ++k) {
    const int c = (lane + 64 * k) * VEC;
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
      const bool ok = lane + 64 * k < nch;
      gam[k][e] = ok ? gamma[c + e] : 0.f;
      bet[k][e] = ok ? beta[c + e] : 0.f;
      pg[k][e] = pgx[k][e] = 0.f;
    }
  }
  const float inv_d = 1.f / (float)D;
  const int64_t r0 = (int64_t)blockIdx.x * rpb;
  for (int rr = wave; rr < rpb; rr += 4) {
    const int64_t r = r0 + rr;
    if (r >= rows) break;  // (wave-uniform)
    float xv[NCH][VEC], gv[NCH][VEC];
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < NCH; ++k) {
      const int64_t off = r * D + (int64_t)(lane + 64 * k) * VEC;
      if (lane + 64 * k < nch) {
        if (H16) {
          const h16x8 xr = *(const h16x8*)((const h16_t*)x + off);
          const h16x8 gr = *(const h16x8*)((const h16_t*)g + off);
#pragma unroll
          for (int e = 0; e < VEC; ++e) {
            xv[k][e] = h2f((h16_t)xr[e]);
            gv[k][e] = h2f((h16_t)gr[e]);
          }
        } else {
          const float4 xr = *(const float4*)((const float*)x + off);
          const float4 gr = *(const float4*)((const float*)g + off);
          xv[k][0] = xr.x, xv[k][1] = xr.y, xv[k][2] = xr.z, xv[k][3] = xr.w;
          gv[k][0] = gr.x, gv[k][1] = gr.y, gv[k][2] = gr.z, gv[k][3] = gr.w;
        }
      } else {
#pragma unroll
        for (int e = 0; e < VEC; ++e) xv[k][e] = gv[k][e] = 0.f;
      }
#pragma unroll
      for (int e = 0; e < VEC; ++e) s += xv[k][e];
    }
    const float mean = wave_sum(s) * inv_d;
    float q = 0.f;
#pragma unroll
    for (int k = 0; k < NCH; ++k)
#pragma unroll
      for (int e = 0; e < VEC; ++e) {
        const float d = lane + 64 * k < nch ? xv[k][e] - mean : 0.f;
        q = fmaf(d, d, q);
      }
    const float rstd = rsqrtf(wave_sum(q) * inv_d + eps);
    float m1 = 0.f, m2 = 0.f;
#pragma unroll
    for (int k = 0; k < NCH; ++k)
#pragma unroll
      for (int e = 0; e < VEC; ++e) {
        // (chunks past D hold x = g = gamma = 0: xhat is -mean rstd there, times a zero gradient)
        const float xh = (xv[k][e] - mean) * rstd;
        const float gg = gv[k][e] * gam[k][e];
        xv[k][e] = xh;
        m1 += gg;
        m2 = fmaf(gg, xh, m2);
        pg[k][e] += gv[k][e];
        pgx[k][e] = fmaf(gv[k][e], xh, pgx[k][e]);
      }
    m1 = wave_sum(m1) * inv_d;
    m2 = wave_sum(m2) * inv_d;
#pragma unroll
    for (int k = 0; k < NCH; ++k) {
      if (lane + 64 * k >= nch) continue;
      const int64_t off = r * D + (int64_t)(lane + 64 * k) * VEC;
      float dv[VEC], zv[VEC];
#pragma unroll
      for (int e = 0; e < VEC; ++e) {
        dv[e] = rstd * (gv[k][e] * gam[k][e] - m1 - xv[k][e] * m2);
        zv[e] = fmaf(xv[k][e], gam[k][e], bet[k][e]);
      }
      if (H16) {
        h16x8 dp, zp;
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
          dp[e] = (short)f2h(dv[e]);
          zp[e] = (short)f2h(zv[e]);
        }
        *(h16x8*)((h16_t*)dx + off) = dp;
        *(h16x8*)((h16_t*)z + off) = zp;
      } else {
        *(float4*)((float*)dx + off) = make_float4(dv[0], dv[1], dv[2], dv[3]);
        *(float4*)((float*)z + off) = make_float4(zv[0], zv[1], zv[2], zv[3]);
      }
    }
  }
#pragma unroll
  for (int k = 0; k < NCH; ++k)
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
      red[wave][0][(lane + 64 * k) * VEC + e] = pg[k][e];
      red[wave][1][(lane + 64 * k) * VEC + e] = pgx[k][e];
    }
  __syncthreads();
  for (int c = threadIdx.x; c < D; c += 256) {
    float tg = 0.f, tx = 0.f;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      tg += red[w][0][c];
      tx += red[w][1][c];
    }
    partials[(int64_t)blockIdx.x * 2 * D + c] = tg;
    partials[(int64_t)blockIdx.x * 2 * D + D + c] = tx;
  }
}

extern "C" int64_t rf_layernorm_bwd_fused_ws_bytes(int64_t rows, int D) {
  if (rows <= 0 || D <= 0) return 0;
  return (int64_t)cdiv(rows, lnf_rows_per_block(rows)) * 2 * D * (int64_t)sizeof(float);
}

extern "C" int rf_layernorm_bwd_fused(const void* x, const void* g, int dtype, const float* gamma, const float* beta, float eps,
                                      void* dx, void* z, float* dgamma, float* dbeta, int accumulate, int64_t rows, int D,
                                      void* workspace, int64_t ws_bytes, void* stream) {
  RF_CHECK_DT(dtype);
  if (!x || !g || !gamma || !beta || !dx || !z || rows <= 0 || D <= 0 || D > LNF_MAXD) return RF_EINVAL;
  if (!workspace || ws_bytes < rf_layernorm_bwd_fused_ws_bytes(rows, D)) return RF_EINVAL;
  // 16-byte row pieces: rows of whole vectors, 16-byte aligned bases
  if (D % (dtype == RF_F32 ? 4 : 8) || ((uintptr_t)x % 16) || ((uintptr_t)g % 16) || ((uintptr_t)dx % 16) || ((uintptr_t)z % 16))
    return RF_EALIGN;
  hipStream_t s = (hipStream_t)stream;
  const int rpb = lnf_rows_per_block(rows);
  const unsigned nblk = cdiv(rows, rpb);
  if (dtype == RF_F32)
    hipLaunchKernelGGL(layernorm_bwd_fused_kernel<false>, dim3(nblk), dim3(256), 0, s, x, g, gamma, beta, eps, dx, z,
                       (float*)workspace, rows, D, rpb);
  else
    hipLaunchKernelGGL(layernorm_bwd_fused_kernel<true>, dim3(nblk), dim3(256), 0, s, x, g, gamma, beta, eps, dx, z,
                       (float*)workspace, rows, D, rpb);
  hipLaunchKernelGGL(layernorm_bwd_finalize_kernel, dim3(cdiv(2 * D, 256)), dim3(256), 0, s, (const float*)workspace, dgamma,
                     dbeta, (int)nblk, D, accumulate ? 1 : 0);
  return rf_launch_status();
}

// ================================================================================================
// rf_absmax: out[0] = max |x[e]| (fp32; NaN propagates); max is order independent, the two passes keep it atomics-free
// ================================================================================================
#define AMAX_BLOCKS 1024

__global__ __launch_bounds__(256) void absmax_kernel(const float* x, int64_t n, float* part) {
  __shared__ float red[4];
  float m = 0.f;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (int64_t)gridDim.x * 256) {
    const float v = fabsf(x[e]);
    m = v > m || v != v ? v : m;
  }
  m = wave_max(m);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) part[blockIdx.x] = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}

extern "C" int rf_absmax(const float* x, int64_t n, float* out, void* workspace, int64_t ws_bytes, void* stream) {
  if (!x || !out || n <= 0) return RF_EINVAL;
  if (!workspace || ws_bytes < AMAX_BLOCKS * (int64_t)sizeof(float)) return RF_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  const unsigned nb = min(cdiv(n, 256), (unsigned)AMAX_BLOCKS);
  hipLaunchKernelGGL(absmax_kernel, dim3(nb), dim3(256), 0, s, x, n, (float*)workspace);
  hipLaunchKernelGGL(absmax_kernel, dim3(1), dim3(256), 0, s, (const float*)workspace, (int64_t)nb, out);
  return rf_launch_status();
}

// ================================================================================================
// pair axial attention backward (model.py PerformerSelfAttention / FeedForward, rf.py:501-528): the elementwise pieces the
// unfused forward chain does not have.  Every product of the FAVOR+ / feed-forward backward runs on rf_gemm / rf_conv_wgrad.
// ================================================================================================

// rf_linattn_normalize_bwd: one wave per row.  out = N[:, :dh] / den, den = N[:, dh]:
//   dN[:, :dh] = g / den,  dN[:, dh] = -sum_c g out / den,  dN[:, dh + 1 .. dn_ld) = 0
__global__ __launch_bounds__(256) void linattn_normalize_bwd_kernel(const float* __restrict__ num, int64_t num_ld,
                                                                    const float* __restrict__ g, int64_t g_ld, void* dn, int dn_dt,
                                                                    int64_t dn_ld, int64_t rows, int dh) {
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= rows) return;  // (wave-uniform)
  const float den = num[r * num_ld + dh];
  const float gv = lane < dh ? g[r * g_ld + lane] : 0.f;
  const float ov = lane < dh ? num[r * num_ld + lane] / den : 0.f;
  const float s = wave_sum(gv * ov);
  for (int c = lane; c < dn_ld; c += 64) {
    const float v = c < dh ? gv / den : (c == dh ? -s / den : 0.f);
    st(dn, dn_dt, r * dn_ld + c, v);
  }
}

extern "C" int rf_linattn_normalize_bwd(const float* num, int64_t num_ld, const float* g, int64_t g_ld, void* dnum, int dtype,
                                        int64_t dnum_ld, int64_t rows, int dh, void* stream) {
  RF_CHECK_DT(dtype);
  if (!num || !g || !dnum || rows <= 0 || dh <= 0 || dh > 64 || num_ld <= dh || g_ld < dh || dnum_ld <= dh) return RF_EINVAL;
  hipLaunchKernelGGL(linattn_normalize_bwd_kernel, dim3(cdiv(rows, 4)), dim3(256), 0, (hipStream_t)stream, num, num_ld, g, g_ld,
                     dnum, dtype, dnum_ld, rows, dh);
  return rf_launch_status();
}

// rf_relu_feature_bwd: dz[r][c] = c < nvalid && z[r][c] > 0 ? dphi[r][c] : 0   (rows x ld, fp32 in, dz of dtype)
__global__ __launch_bounds__(256) void relu_feature_bwd_kernel(const float* __restrict__ dphi, const float* __restrict__ z, void* dz,
                                                               int dz_dt, int ld_, int nvalid, int64_t total) {
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
    const int c = (int)(e % ld_);
    st(dz, dz_dt, e, c < nvalid && z[e] > 0.f ? dphi[e] : 0.f);
  }
}

extern "C" int rf_relu_feature_bwd(const float* dphi, const float* z, void* dz, int dtype, int64_t rows, int ld, int nvalid,
                                   void* stream) {
  RF_CHECK_DT(dtype);
  if (!dphi || !z || !dz || rows <= 0 || ld <= 0 || nvalid < 0 || nvalid > ld) return RF_EINVAL;
  const int64_t total = rows * ld;
  hipLaunchKernelGGL(relu_feature_bwd_kernel, dim3(min(cdiv(total, 256), 16384u)), dim3(256), 0, (hipStream_t)stream, dphi, z, dz,
                     dtype, ld, nvalid, total);
  return rf_launch_status();
}

// rf_relu_dropout_bwd: dh[e] = h[e] > 0 ? g[e] * (keep(seed, offset, e) ? 1 / (1 - p) : 0) : 0   (p = 0: no mask)
__global__ __launch_bounds__(256) void relu_dropout_bwd_kernel(const float* __restrict__ g, const float* __restrict__ h, void* dh,
                                                               int dh_dt, int drop, unsigned thresh, float inv_keep, uint64_t seed,
                                                               uint64_t offset, int64_t n) {
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (int64_t)gridDim.x * 256) {
    float v = h[e] > 0.f ? g[e] : 0.f;
    if (drop) v = dropout_keep(seed, offset, e, thresh) ? v * inv_keep : 0.f;
    st(dh, dh_dt, e, v);
  }
}

extern "C" int rf_relu_dropout_bwd(const float* g, const float* h, void* dh, int dtype, float p, uint64_t seed, uint64_t offset,
                                   int64_t n, void* stream) {
  RF_CHECK_DT(dtype);
  if (!g || !h || !dh || n < 0 || !(p >= 0.f) || !(p < 1.f)) return RF_EINVAL;
  if (n == 0) return 0;
  hipLaunchKernelGGL(relu_dropout_bwd_kernel, dim3(min(cdiv(n, 256), 16384u)), dim3(256), 0, (hipStream_t)stream, g, h, dh, dtype,
                     p > 0.f ? 1 : 0, dropout_threshold(p), 1.f / (1.f - p), seed, offset, n);
  return rf_launch_status();
}

// ================================================================================================
// rf_graph_attention_bwd: backward of the GraphTransformer attention core (ops.hip: graph_attention_kernel and its masked /
// dropout forms; rf.py:647-662).  Block per row (b, i) like the forward; the row's logits and probabilities are recomputed
// (the forward saves nothing of size L * L).  With HD = H * d channels a block of 256 threads holds G = 256 / HD column
// groups: thread (cg, c) owns channel c of the columns n = cg, cg + G, ...
//   phase 0  the row's ascending column list idx[] and its inverse pos[] (the forward's compaction; NULL mask: the identity)
//   phase 1  one pass over the row's e: s_n = scale q.(k_j + e_ij) and dpd_n = g.(v_j + e_ij), j = idx[n]
//   phase 2  per head, one wave: p = softmax(s), dp = keep / (1 - p_drop) dpd, ds = p (dp - sum p dp), pd = keep / (1 - p_drop) p
//   phase 3  the maps pd, ds [B, H, L, map_ld] fp32, zeros at masked columns and in the pad columns
//   phase 4  second pass over the row's e (L2): dq_i = scale sum ds_n (k_j + e_ij), de_ij = pd g_i + scale ds q_i (0 at a
//            masked column); the G partial dq are added in group order through LDS
// A row with no edge: every logit is the constant 0, so ds = 0 and dq = 0 exactly, de_ij = pd_j g_i with p = 1 / L, and
// k, v, e are not read.  graph_attention_bwd_cols_kernel then takes the sums across rows, dv_j = sum_i pd_ij g_i and
// dk_j = scale sum_i ds_ij q_i, from the maps in row order: no atomics, the same bits run to run.
// ================================================================================================
#define GAB_JT 2  // columns per block of the cross-row kernel

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

static inline size_t gab_lds_bytes(int L, int H) { return ((size_t)2 * H * L + 2 * (size_t)L + 8 + 512) * sizeof(float); }

template <bool DROP>
__global__ __launch_bounds__(256) void graph_attention_bwd_kernel(const void* q, const void* k, const void* v, const void* e, int dt,
                                                                  const uint8_t* mask, const float* __restrict__ g,
                                                                  float* __restrict__ dq, void* de, float* __restrict__ pd_map,
                                                                  float* __restrict__ ds_map, int map_ld, int L, int H, int d,
                                                                  float scale, unsigned thresh, float inv_keep, uint64_t seed,
                                                                  uint64_t offset) {
  extern __shared__ __attribute__((aligned(16))) float gab_sm[];
  float* sp = gab_sm;                  // [H][L]: logits, then p, then pd   (row h holds deg entries)
  float* sd = sp + (size_t)H * L;      // [H][L]: dpd, then dp, then ds
  int* idx = (int*)(sd + (size_t)H * L);  // [L]: n -> column
  int* pos = idx + L;                  // [L]: column -> n, -1 at a masked column
  int* wcnt = pos + L;                 // [8]: edges found by each wave in a 256-column chunk
  double* red = (double*)(wcnt + 8);   // [256]: the column groups' partial dq (8-byte aligned: every count above is even)
  const int bi = blockIdx.x, b = bi / L, i = bi % L;
  const int HD = H * d;
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const int G = 256 / HD;
  const int cg = t / HD, c = t - cg * HD;
  const bool act = cg < G;
  const int h = c / d;  // (a head's d lanes are lane-aligned: HD and 64 are multiples of d)
  // ---- phase 0
  bool empty = false;  // block-uniform
  int deg = L;
  if (mask) {
    const uint8_t* mrow = mask + (int64_t)bi * L;
    int found = 0;
    for (int c0 = 0; c0 < L; c0 += 256) {
      const int j = c0 + t;
      const bool on = j < L && mrow[j] != 0;
      const unsigned long long bal = __ballot(on);
      if (lane == 0) wcnt[wv] = __popcll(bal);
      __syncthreads();
      const int w0 = wcnt[0], w1 = wcnt[1], w2 = wcnt[2], w3 = wcnt[3];
      const int before = found + (wv > 0 ? w0 : 0) + (wv > 1 ? w1 : 0) + (wv > 2 ? w2 : 0);
      if (on) {
        const int n = before + __popcll(bal & ((1ull << lane) - 1ull));
        idx[n] = j;
        pos[j] = n;
      } else if (j < L) {
        pos[j] = -1;
      }
      found += w0 + w1 + w2 + w3;
      __syncthreads();  // wcnt is rewritten by the next chunk
    }
    empty = found == 0;
    deg = empty ? L : found;
  }
  if (!mask || empty)
    for (int n = t; n < L; n += 256) idx[n] = pos[n] = n;
  __syncthreads();
  // ---- phase 1
  const float qv = act ? ld(q, dt, (int64_t)bi * HD + c) : 0.f;
  const float gv = act ? g[(int64_t)bi * HD + c] : 0.f;
  if (empty) {
    for (int x = t; x < H * L; x += 256) sp[x] = sd[x] = 0.f;
  } else {
    for (int n0 = 0; n0 < deg; n0 += G) {  // (block-uniform trip count: the shuffles below run with every lane)
      const int n = n0 + cg;
      const bool ok = act && n < deg;
      float s = 0.f, dp = 0.f;
      if (ok) {
        const int j = idx[n];
        const float ev = ld(e, dt, ((int64_t)bi * L + j) * HD + c);
        s = qv * (ld(k, dt, ((int64_t)b * L + j) * HD + c) + ev);
        dp = gv * (ld(v, dt, ((int64_t)b * L + j) * HD + c) + ev);
      }
      for (int o = d >> 1; o > 0; o >>= 1) {
        s += __shfl_xor(s, o, 64);
        dp += __shfl_xor(dp, o, 64);
      }
      if (ok && (c % d) == 0) {
        sp[h * L + n] = s * scale;
        sd[h * L + n] = dp;
      }
    }
  }
  __syncthreads();
  // ---- phase 2 (a lane reads and writes its own entries n = lane + 64 m only)
  for (int hh = wv; hh < H; hh += 4) {
    float* ps = sp + hh * L;
    float* pg = sd + hh * L;
    const int64_t el0 = (((int64_t)b * H + hh) * L + i) * L;  // element [b, hh, i, 0] of the forward's dropout map
    float mx = -INFINITY;
    for (int n = lane; n < deg; n += 64) mx = fmaxf(mx, ps[n]);
    mx = wave_max(mx);
    // The normaliser, sum p dp and dp - sum p dp are taken in fp64 (H * L scalars per row, against H * d * L channel terms): the
    // probabilities then add up to one to fp64 accuracy, and the cancellation in ds, which grows like 1 / (1 - max p) in a row of
    // two or three edges, loses nothing beyond the fp32 rounding of the logits themselves.
    double s = 0.0;
    for (int n = lane; n < deg; n += 64) {
      const float ex = expf(ps[n] - mx);
      ps[n] = ex;
      s += (double)ex;
    }
    const double inv = 1.0 / wave_sum_f64(s);
    double dot = 0.0;
    for (int n = lane; n < deg; n += 64) {
      float dp = pg[n];
      if (DROP) dp = dropout_keep(seed, offset, el0 + idx[n], thresh) ? dp * inv_keep : 0.f;
      dot = fma((double)ps[n] * inv, (double)dp, dot);
      pg[n] = dp;
    }
    dot = wave_sum_f64(dot);
    for (int n = lane; n < deg; n += 64) {
      const double pr = (double)ps[n] * inv;
      pg[n] = (float)(pr * ((double)pg[n] - dot));
      float pd = (float)pr;
      if (DROP) pd = dropout_keep(seed, offset, el0 + idx[n], thresh) ? pd * inv_keep : 0.f;
      ps[n] = pd;
    }
  }
  __syncthreads();
  // ---- phase 3
  for (int x = t; x < H * map_ld; x += 256) {
    const int hh = x / map_ld, j = x - hh * map_ld;
    const int n = j < L ? pos[j] : -1;
    const int64_t o = (((int64_t)b * H + hh) * L + i) * map_ld + j;
    pd_map[o] = n >= 0 ? sp[hh * L + n] : 0.f;
    ds_map[o] = n >= 0 ? sd[hh * L + n] : 0.f;
  }
  // ---- phase 4
  double a = 0.0;  // (fp64: one fused multiply-add per column next to three loads and a store)
  for (int j0 = 0; j0 < L; j0 += G) {
    const int j = j0 + cg;
    if (act && j < L) {
      const int n = pos[j];
      float dev = 0.f;
      if (n >= 0) {
        const float dsv = sd[h * L + n];
        dev = sp[h * L + n] * gv;
        if (!empty) {
          a = fma((double)dsv, (double)ld(k, dt, ((int64_t)b * L + j) * HD + c) + (double)ld(e, dt, ((int64_t)bi * L + j) * HD + c), a);
          dev = fmaf(scale * dsv, qv, dev);
        }
      }
      st(de, dt, ((int64_t)bi * L + j) * HD + c, dev);
    }
  }
  red[t] = a;
  __syncthreads();
  if (t < HD) {
    double s = 0.0;
    for (int x = 0; x < G; ++x) s += red[x * HD + t];
    dq[(int64_t)bi * HD + t] = (float)((double)scale * s);
  }
}

// dv[b, j, c] = sum_i pd[b, h, i, j] g[b, i, c],  dk[b, j, c] = scale sum_i ds[b, h, i, j] q[b, i, c]:
// block = GAB_JT columns of one sample; thread (ig, c) sums channel c of head h over the rows i = ig, ig + G, ... (ascending,
// fp64: the kernel waits on its loads, not on its arithmetic), and the G = 256 / HD partial sums meet in LDS in group order
__global__ __launch_bounds__(256) void graph_attention_bwd_cols_kernel(const float* __restrict__ pd_map, const float* __restrict__ ds_map,
                                                                       int map_ld, const float* __restrict__ g, const void* q, int dt,
                                                                       float* __restrict__ dk, float* __restrict__ dv, int L, int H,
                                                                       int d, int tiles, float scale) {
  __shared__ double red[2 * GAB_JT][256];
  const int HD = H * d, t = threadIdx.x;
  const int G = 256 / HD;
  const int ig = t / HD, c = t - ig * HD;
  const int b = blockIdx.x / tiles, j0 = (blockIdx.x % tiles) * GAB_JT;
  const int h = c / d;
  double av[GAB_JT], ak[GAB_JT];
#pragma unroll
  for (int u = 0; u < GAB_JT; ++u) av[u] = ak[u] = 0.0;
  if (ig < G) {
    const int64_t m0 = ((int64_t)b * H + h) * L * map_ld + j0;
#pragma unroll 4
    for (int i = ig; i < L; i += G) {
      const float gv = g[((int64_t)b * L + i) * HD + c];
      const float qv = ld(q, dt, ((int64_t)b * L + i) * HD + c);
#pragma unroll
      for (int u = 0; u < GAB_JT; ++u)
        if (j0 + u < L) {
          av[u] = fma((double)pd_map[m0 + (int64_t)i * map_ld + u], (double)gv, av[u]);
          ak[u] = fma((double)ds_map[m0 + (int64_t)i * map_ld + u], (double)qv, ak[u]);
        }
    }
  }
#pragma unroll
  for (int u = 0; u < GAB_JT; ++u) {
    red[u][t] = av[u];
    red[GAB_JT + u][t] = ak[u];
  }
  __syncthreads();
  if (t < HD) {
#pragma unroll
    for (int u = 0; u < GAB_JT; ++u)
      if (j0 + u < L) {
        double sv = 0.0, sk = 0.0;
        for (int x = 0; x < G; ++x) {
          sv += red[u][x * HD + t];
          sk += red[GAB_JT + u][x * HD + t];
        }
        dv[((int64_t)b * L + j0 + u) * HD + t] = (float)sv;
        dk[((int64_t)b * L + j0 + u) * HD + t] = (float)((double)scale * sk);
      }
  }
}

// include/rfmi.h: rf_graph_attention_bwd
extern "C" int rf_graph_attention_bwd(const void* q, const void* k, const void* v, const void* e, int dtype, const uint8_t* mask,
                                      const float* g, float* dq, float* dk, float* dv, void* de, float* pd_map, float* ds_map,
                                      int64_t map_ld, int B, int L, int H, int d, float scale, float p, uint64_t seed,
                                      uint64_t offset, void* stream) {
  RF_CHECK_DT(dtype);
  if (!q || !k || !v || !e || !g || !dq || !dk || !dv || !de || !pd_map || !ds_map) return RF_EINVAL;
  if (B <= 0 || L <= 0 || H <= 0 || d <= 0 || H * d > 256 || d > 64 || (d & (d - 1)) != 0) return RF_EINVAL;
  if (!(p >= 0.f) || !(p < 1.f)) return RF_EINVAL;
  if (map_ld < L || (int64_t)H * map_ld > 0x7fffffff || (int64_t)B * L > 0x7fffffff) return RF_EINVAL;
  const size_t lds = gab_lds_bytes(L, H);
  if (lds > 64 * 1024) return RF_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  if (p > 0.f)
    hipLaunchKernelGGL(graph_attention_bwd_kernel<true>, dim3(B * L), dim3(256), lds, s, q, k, v, e, dtype, mask, g, dq, de, pd_map,
                       ds_map, (int)map_ld, L, H, d, scale, dropout_threshold(p), 1.f / (1.f - p), seed, offset);
  else
    hipLaunchKernelGGL(graph_attention_bwd_kernel<false>, dim3(B * L), dim3(256), lds, s, q, k, v, e, dtype, mask, g, dq, de, pd_map,
                       ds_map, (int)map_ld, L, H, d, scale, 0u, 1.f, (uint64_t)0, (uint64_t)0);
  const int tiles = (int)cdiv(L, GAB_JT);
  hipLaunchKernelGGL(graph_attention_bwd_cols_kernel, dim3((unsigned)B * tiles), dim3(256), 0, s, pd_map, ds_map,
                     (int)map_ld, g, q, dtype, dk, dv, L, H, d, tiles, scale);
  return rf_launch_status();
}

// rf_elu_bwd: da[e] = g[e] * (a > 0 ? 1 : a + 1), a = y[e] - x[e] the ELU's value (x NULL: a = y[e])
__global__ __launch_bounds__(256) void elu_bwd_kernel(const float* __restrict__ g, const float* __restrict__ y,
                                                      const float* __restrict__ x, void* da, int da_dt, int64_t n) {
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (int64_t)gridDim.x * 256) {
    const float a = x ? y[e] - x[e] : y[e];
    st(da, da_dt, e, g[e] * (a > 0.f ? 1.f : a + 1.f));
  }
}

extern "C" int rf_elu_bwd(const float* g, const float* y, const float* x, void* da, int dtype, int64_t n, void* stream) {
  RF_CHECK_DT(dtype);
  if (!g || !y || !da || n < 0) return RF_EINVAL;
  if (n == 0) return 0;
  hipLaunchKernelGGL(elu_bwd_kernel, dim3(min(cdiv(n, 256), 16384u)), dim3(256), 0, (hipStream_t)stream, g, y, x, da, dtype, n);
  return rf_launch_status();
}

// ================================================================================================
// rf_poswise_bwd: backward of PositionWiseWeightFactor's core (ops.hip: poswise_kernel; rf.py:205-217), optionally with the
// weighted sum over the MSA depth (weighted_msa_sum_kernel; rf.py:723) fused behind it.  Block per (b, l) like the forward; the
// logits and the weights are recomputed from q0 and k.  A chunk is CH = 8 channels (16-byte accesses) or one channel (the
// scalar path: any dlen, any alignment; the host chooses).
//   phase 1  one pass over the block's k rows: logit_{n,h} = scale q0_h . k_{n,h} and, fused form, z_n = k_n . ds.  A group of
//            G lanes (a power of two, the chunks of one head) owns one (n, h) and meets in a shuffle reduction
//   phase 2  per head, one wave: w = softmax(logit), dw = keep / (1 - p) (dw + z), dlogit = w (dw - sum w dw),
//            wd = keep / (1 - p) w
//   phase 3  second pass over k (L2): thread (rg, cc) owns chunk cc of the H * dlen / CH column chunks and walks the rows
//            n = rg, rg + R, ...: dk_n = scale dlogit_n q0 + wd_n ds, and its partial dq0 = sum_n dlogit_n k_n; the R partial
//            sums are added in group order through LDS
// N == 1: w = 1 and dw - sum w dw = 0 exactly, so dlogit = 0, dq0 = 0, dk = wd ds.
// ================================================================================================
template <bool VEC>
__device__ __forceinline__ void pwb_load(const void* p, int dt, int64_t o, float (&v)[VEC ? 8 : 1]) {
  if constexpr (VEC) {
    if (dt == RF_F32) {
      const float4 a = *(const float4*)((const float*)p + o), b = *(const float4*)((const float*)p + o + 4);
      v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
      v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
    } else {
      const h16x8 a = *(const h16x8*)((const h16_t*)p + o);
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] = h2f((h16_t)a[e]);
    }
  } else {
    v[0] = ld(p, dt, o);
  }
}

template <bool VEC>
__device__ __forceinline__ void pwb_store(void* p, int dt, int64_t o, const float (&v)[VEC ? 8 : 1]) {
  if constexpr (VEC) {
    if (dt == RF_F32) {
      *(float4*)((float*)p + o) = make_float4(v[0], v[1], v[2], v[3]);
      *(float4*)((float*)p + o + 4) = make_float4(v[4], v[5], v[6], v[7]);
    } else {
      h16x8 a;
#pragma unroll
      for (int e = 0; e < 8; ++e) a[e] = (short)f2h(v[e]);
      *(h16x8*)((h16_t*)p + o) = a;
    }
  } else {
    st(p, dt, o, v[0]);
  }
}

static inline size_t pwb_lds_bytes(int N, int H) { return ((size_t)2 * N * H + 512) * sizeof(float); }

template <bool VEC, bool DROP>
__global__ __launch_bounds__(256) void poswise_bwd_kernel(const void* q0, int q0_dt, int64_t q0_ld, const void* k, int dt,
                                                          int64_t k_ld, int k_col0, int k_hs, int dlen,
                                                          const float* __restrict__ dw, const float* __restrict__ ds, int64_t ds_ld,
                                                          float* __restrict__ dq0, void* dk, int dk_dt, int64_t dk_ld, int dk_col0,
                                                          int dk_hs, int N, int L, int H, float scale, unsigned thresh,
                                                          float inv_keep, uint64_t seed, uint64_t offset) {
  constexpr int CH = VEC ? 8 : 1;
  extern __shared__ __attribute__((aligned(16))) float pwb_sm[];
  double* red = (double*)pwb_sm;         // [256]: the row groups' partial dq0 of one channel
  float* sl = pwb_sm + 512;              // [H][N]: logits, then exp, then wd
  float* sd = sl + (size_t)N * H;        // [H][N]: z, then dw, then dlogit
  const int bl = blockIdx.x, b = bl / L, l = bl - b * L;
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const int NH = N * H;
  const int nch = (dlen + CH - 1) / CH;  // chunks of one head
  const int64_t qrow = (int64_t)bl * q0_ld, dsrow = (int64_t)bl * ds_ld;
  // ---- phase 1
  {
    int G = 1;
    while (G < nch && G < 64) G <<= 1;
    const int ipp = 256 / G, gi = t / G, gj = t & (G - 1);
    for (int i0 = 0; i0 < NH; i0 += ipp) {  // (block-uniform trip count: the shuffles below run with every lane)
      const int item = i0 + gi;
      const bool ok = item < NH;
      const int n = item / H, h = item - n * H;
      float a = 0.f, z = 0.f;
      if (ok) {
        const int64_t kb = (((int64_t)b * N + n) * L + l) * k_ld + k_col0 + (int64_t)h * k_hs;
        const int64_t qb = qrow + (int64_t)h * dlen;
        for (int c = gj; c < nch; c += G) {
          float kv[CH], qv[CH];
          pwb_load<VEC>(k, dt, kb + (int64_t)c * CH, kv);
          pwb_load<VEC>(q0, q0_dt, qb + (int64_t)c * CH, qv);
#pragma unroll
          for (int e = 0; e < CH; ++e) a = fmaf(qv[e], kv[e], a);
          if (ds) {
            float dv[CH];
            pwb_load<VEC>(ds, RF_F32, dsrow + (int64_t)c * CH, dv);
#pragma unroll
            for (int e = 0; e < CH; ++e) z = fmaf(dv[e], kv[e], z);
          }
        }
      }
      for (int o = G >> 1; o > 0; o >>= 1) {
        a += __shfl_xor(a, o, 64);
        z += __shfl_xor(z, o, 64);
      }
      if (ok && gj == 0) {
        sl[h * N + n] = a * scale;
        sd[h * N + n] = z;
      }
    }
  }
  __syncthreads();
  // ---- phase 2 (a lane reads and writes its own entries n = lane + 64 m only)
  for (int hh = wv; hh < H; hh += 4) {
    float* ps = sl + hh * N;
    float* pg = sd + hh * N;
    float mx = -INFINITY;
    for (int n = lane; n < N; n += 64) mx = fmaxf(mx, ps[n]);
    mx = wave_max(mx);
    double s = 0.0;
    for (int n = lane; n < N; n += 64) {
      const float ex = expf(ps[n] - mx);
      ps[n] = ex;
      s += (double)ex;
    }
    const double inv = 1.0 / wave_sum_f64(s);
    double dot = 0.0;
    for (int n = lane; n < N; n += 64) {
      const int64_t el = (((int64_t)b * N + n) * H + hh) * L + l;  // element [b, n, hh, l] of the weights and their dropout mask
      float g = pg[n] + (dw ? dw[el] : 0.f);
      if (DROP) g = dropout_keep(seed, offset, el, thresh) ? g * inv_keep : 0.f;
      dot = fma((double)ps[n] * inv, (double)g, dot);
      pg[n] = g;
    }
    dot = wave_sum_f64(dot);
    for (int n = lane; n < N; n += 64) {
      const double pr = (double)ps[n] * inv;
      pg[n] = (float)(pr * ((double)pg[n] - dot));
      float wd = (float)pr;
      if (DROP) wd = dropout_keep(seed, offset, (((int64_t)b * N + n) * H + hh) * L + l, thresh) ? wd * inv_keep : 0.f;
      ps[n] = wd;
    }
  }
  __syncthreads();
  // ---- phase 3
  const int CC = H * nch;
  const int CCt = CC < 256 ? CC : 256;
  const int R = 256 / CCt;
  const int rg = t / CCt, cl = t - rg * CCt;
  for (int cc0 = 0; cc0 < CC; cc0 += CCt) {  // (block-uniform trip count: the barriers below are met by every thread)
    const int cc = cc0 + cl;
    const bool ok = rg < R && cc < CC;
    const int h = ok ? cc / nch : 0, c = ok ? cc - h * nch : 0;
    double acc[CH];
#pragma unroll
    for (int e = 0; e < CH; ++e) acc[e] = 0.0;
    if (ok) {
      float qv[CH], dv[CH];
      pwb_load<VEC>(q0, q0_dt, qrow + (int64_t)h * dlen + (int64_t)c * CH, qv);
#pragma unroll
      for (int e = 0; e < CH; ++e) dv[e] = 0.f;
      if (ds) pwb_load<VEC>(ds, RF_F32, dsrow + (int64_t)c * CH, dv);
      for (int n = rg; n < N; n += R) {
        const int64_t row = ((int64_t)b * N + n) * L + l;
        float kv[CH], ov[CH];
        pwb_load<VEC>(k, dt, row * k_ld + k_col0 + (int64_t)h * k_hs + (int64_t)c * CH, kv);
        const float dl = sd[h * N + n];
        const double sdl = (double)scale * (double)dl, wd = (double)sl[h * N + n];
#pragma unroll
        for (int e = 0; e < CH; ++e) {
          acc[e] = fma((double)dl, (double)kv[e], acc[e]);
          ov[e] = (float)fma(sdl, (double)qv[e], wd * (double)dv[e]);
        }
        pwb_store<VEC>(dk, dk_dt, row * dk_ld + dk_col0 + (int64_t)h * dk_hs + (int64_t)c * CH, ov);
      }
    }
#pragma unroll
    for (int e = 0; e < CH; ++e) {
      red[t] = acc[e];
      __syncthreads();
      if (ok && rg == 0) {
        double s = 0.0;
        for (int x = 0; x < R; ++x) s += red[x * CCt + cl];
        dq0[(int64_t)bl * H * dlen + (int64_t)h * dlen + (int64_t)c * CH + e] = (float)((double)scale * s);
      }
      __syncthreads();
    }
  }
}

// include/rfmi.h: rf_poswise_bwd
extern "C" int rf_poswise_bwd(const void* q0, int q0_dtype, int64_t q0_ld, const void* k, int dtype, int64_t k_ld, int k_col0,
                              int k_hstride, int dlen, const float* dw, const float* ds, int64_t ds_ld, float* dq0, void* dk,
                              int dk_dtype, int64_t dk_ld, int dk_col0, int dk_hstride, int B, int N, int L, int H, float scale,
                              float p, uint64_t seed, uint64_t offset, void* stream) {
  RF_CHECK_DT(dtype);
  RF_CHECK_DT(q0_dtype);
  RF_CHECK_DT(dk_dtype);
  if (!q0 || !k || !dq0 || !dk || (!dw && !ds)) return RF_EINVAL;
  if (B <= 0 || N <= 0 || L <= 0 || H <= 0 || dlen <= 0 || (int64_t)B * L > 0x7fffffff || (int64_t)N * H > 0x7fffffff) return RF_EINVAL;
  if (k_col0 < 0 || k_hstride < 0 || dk_col0 < 0 || dk_hstride < 0) return RF_EINVAL;
  if (q0_ld < (int64_t)H * dlen || k_ld < k_col0 + (int64_t)(H - 1) * k_hstride + dlen) return RF_EINVAL;
  if (dk_ld < dk_col0 + (int64_t)(H - 1) * dk_hstride + dlen || (H > 1 && dk_hstride < dlen)) return RF_EINVAL;
  if (ds && (H != 1 || ds_ld < dlen)) return RF_EINVAL;
  if (!(p >= 0.f) || !(p < 1.f)) return RF_EINVAL;
  if ((int64_t)N * H > 16384) return RF_EINVAL;
  const size_t lds = pwb_lds_bytes(N, H);
  if (lds > 64 * 1024) return RF_EINVAL;
  const int64_t strides = q0_ld | k_ld | k_col0 | (H > 1 ? k_hstride : 0) | dk_ld | dk_col0 | (H > 1 ? dk_hstride : 0) | (ds ? ds_ld : 0);
  const uintptr_t ptrs = (uintptr_t)q0 | (uintptr_t)k | (uintptr_t)dq0 | (uintptr_t)dk | (uintptr_t)ds;
  const bool vec = (dlen & 7) == 0 && (strides & 7) == 0 && (ptrs & 15) == 0;
  const bool drop = p > 0.f;
  const unsigned thresh = drop ? dropout_threshold(p) : 0u;
  const float inv_keep = drop ? 1.f / (1.f - p) : 1.f;
  if (!drop) seed = offset = 0;
#define PWB_LAUNCH(V_, D_)                                                                                                          \
  hipLaunchKernelGGL((poswise_bwd_kernel<V_, D_>), dim3(B * L), dim3(256), lds, (hipStream_t)stream, q0, q0_dtype, q0_ld, k, dtype, \
                     k_ld, k_col0, k_hstride, dlen, dw, ds, ds_ld, dq0, dk, dk_dtype, dk_ld, dk_col0, dk_hstride, N, L, H, scale,   \
                     thresh, inv_keep, seed, offset)
  if (vec && drop) PWB_LAUNCH(true, true);
  else if (vec) PWB_LAUNCH(true, false);
  else if (drop) PWB_LAUNCH(false, true);
  else PWB_LAUNCH(false, false);
#undef PWB_LAUNCH
  return rf_launch_status();
}

// ================================================================================================
// rf_dist_masked_attention_bwd: backward of MsaUpdateWithPairAndCoord's attention map (ops.hip: dist_att_kernel; rf.py:899-914).
// Block per row (b, i) like the forward, with the forward's LDS (H * L floats and nothing more); the row's logits and
// probabilities are recomputed from q, k and xyz (the stored map is 16-bit and is not read).
//   phase 1  the forward's own loop: logit_{h,j} = q_i . k_j + dist_mask_bias (common.h: the same fp32 decision as the forward)
//   phase 2  per head, one wave: p = softmax(logit), ds = p (datt - sum p datt); datt is streamed from memory twice (the second
//            time from cache) instead of doubling the LDS; ds replaces p in LDS and goes to the fp32 map ds_map [B, H, L, L]
//   phase 3  dq_i = sum_j ds_j k_j: a wave takes DAB_CW channels at a time, its 64 / DAB_CW lane groups split j (ascending within
//            a group) and meet in a shuffle butterfly -- no scratch beyond the forward's LDS
// dist_att_bwd_cols_kernel, block per (b, j), then sums dk_j = sum_i ds_ij q_i from the map the same way: no atomics, a fixed
// order, the same bits run to run.  A masked entry has exp(-1e9 - max) = 0, so p = 0 and ds = 0 exactly.
// ================================================================================================
#define DAB_CW 16  // channels a wave takes at a time (64-byte segments of a k / q row); 64 / DAB_CW lane groups split the sum

__global__ __launch_bounds__(256) void dist_att_bwd_kernel(const float* __restrict__ q, const float* __restrict__ k,
                                                           const float* __restrict__ xyz, const float* __restrict__ bins,
                                                           const float* __restrict__ datt, float* __restrict__ dq,
                                                           float* __restrict__ ds_map, int L, int H, int d) {
  extern __shared__ float dab_sm[];  // [H][L]: logits, then exp, then ds
  const int bi = blockIdx.x, b = bi / L, i = bi - b * L;
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const int HD = H * d;
  // ---- phase 1
  const float cx = xyz[((int64_t)bi * 3 + 1) * 3 + 0], cy = xyz[((int64_t)bi * 3 + 1) * 3 + 1],
              cz = xyz[((int64_t)bi * 3 + 1) * 3 + 2];
  for (int e = t; e < H * L; e += 256) {
    const int h = e / L, j = e - h * L;
    const float* qr = q + ((int64_t)bi * H + h) * d;
    const float* kr = k + (((int64_t)b * L + j) * H + h) * d;
    float a = 0.f;
    for (int c = 0; c < d; ++c) a = fmaf(qr[c], kr[c], a);
    dab_sm[e] = a + dist_mask_bias(cx, cy, cz, xyz + (((int64_t)b * L + j) * 3 + 1) * 3, bins[h]);
  }
  __syncthreads();
  // ---- phase 2 (a lane reads and writes its own entries j = lane + 64 m only)
  for (int h = wv; h < H; h += 4) {
    float* ps = dab_sm + h * L;
    const int64_t row = (((int64_t)b * H + h) * L + i) * L;  // element [b, h, i, 0] of datt and of the map
    float mx = -INFINITY;
    for (int j = lane; j < L; j += 64) mx = fmaxf(mx, ps[j]);
    mx = wave_max(mx);
    // the normaliser and sum p datt in fp64, as in graph_attention_bwd_kernel: a row with two or three residues in range
    // cancels in datt - sum p datt
    double s = 0.0;
    for (int j = lane; j < L; j += 64) {
      const float ex = expf(ps[j] - mx);
      ps[j] = ex;
      s += (double)ex;
    }
    const double inv = 1.0 / wave_sum_f64(s);
    double dot = 0.0;
    for (int j = lane; j < L; j += 64) dot = fma((double)ps[j] * inv, (double)datt[row + j], dot);
    dot = wave_sum_f64(dot);
    for (int j = lane; j < L; j += 64) {
      const float dsv = (float)((double)ps[j] * inv * ((double)datt[row + j] - dot));
      ps[j] = dsv;
      ds_map[row + j] = dsv;
    }
  }
  __syncthreads();
  // ---- phase 3
  const int jg = lane / DAB_CW, cl = lane % DAB_CW;
  const int nchunk = (HD + DAB_CW - 1) / DAB_CW;
  for (int ch = wv; ch < nchunk; ch += 4) {  // (wave-uniform trip count: the shuffles below run with every lane)
    const int c = ch * DAB_CW + cl;
    const bool ok = c < HD;
    double a = 0.0;
    if (ok) {
      const float* ds = dab_sm + (c / d) * L;
      const float* kc = k + (int64_t)b * L * HD + c;
#pragma unroll 4
      for (int j = jg; j < L; j += 64 / DAB_CW) a = fma((double)ds[j], (double)kc[(int64_t)j * HD], a);
    }
    for (int o = DAB_CW; o < 64; o <<= 1) a += __shfl_xor(a, o, 64);
    if (ok && jg == 0) dq[(int64_t)bi * HD + c] = (float)a;
  }
}

// dk[b, j, c] = sum_i ds[b, h, i, j] q[b, i, c]: block per (b, j); lanes and order as in phase 3 above, over the rows i
__global__ __launch_bounds__(256) void dist_att_bwd_cols_kernel(const float* __restrict__ ds_map, const float* __restrict__ q,
                                                                float* __restrict__ dk, int L, int H, int d) {
  const int bj = blockIdx.x, b = bj / L, j = bj - b * L;
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const int HD = H * d;
  const int ig = lane / DAB_CW, cl = lane % DAB_CW;
  const int nchunk = (HD + DAB_CW - 1) / DAB_CW;
  for (int ch = wv; ch < nchunk; ch += 4) {
    const int c = ch * DAB_CW + cl;
    const bool ok = c < HD;
    double a = 0.0;
    if (ok) {
      const float* col = ds_map + ((int64_t)b * H + c / d) * L * L + j;
      const float* qc = q + (int64_t)b * L * HD + c;
#pragma unroll 4
      for (int i = ig; i < L; i += 64 / DAB_CW) a = fma((double)col[(int64_t)i * L], (double)qc[(int64_t)i * HD], a);
    }
    for (int o = DAB_CW; o < 64; o <<= 1) a += __shfl_xor(a, o, 64);
    if (ok && ig == 0) dk[(int64_t)bj * HD + c] = (float)a;
  }
}

// include/rfmi.h: rf_dist_masked_attention_bwd
extern "C" int rf_dist_masked_attention_bwd(const float* q, const float* k, const float* xyz, const float* bins, const float* datt,
                                            float* dq, float* dk, float* ds_map, int B, int L, int H, int d, void* stream) {
  if (!q || !k || !xyz || !bins || !datt || !dq || !dk || !ds_map) return RF_EINVAL;
  if (B <= 0 || L <= 0 || H <= 0 || d <= 0 || (int64_t)B * L > 0x7fffffff || (int64_t)H * d > 0x7fffffff) return RF_EINVAL;
  const size_t lds = (size_t)H * L * sizeof(float);  // the forward's
  if (lds > 64 * 1024) return RF_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(dist_att_bwd_kernel, dim3(B * L), dim3(256), lds, s, q, k, xyz, bins, datt, dq, ds_map, L, H, d);
  hipLaunchKernelGGL(dist_att_bwd_cols_kernel, dim3(B * L), dim3(256), 0, s, ds_map, q, dk, L, H, d);
  return rf_launch_status();
}

// ================================================================================================
// rf_tied_softmax_bwd: backward of the tied attention's softmax and of its symmetrised map (ops.hip: softmax_kernel and
// att_sym_kernel; rf.py:255, 261-265).  Per (b, h, i), over the columns j:
//   p = softmax_j(logits),   dp_j = dp[b,h,i,j] + (g_sym[b,i,j,h] + g_sym[b,j,i,h]) / 2,   ds_j = p_j (dp_j - sum_l p_l dp_l)
// A block takes TI query rows i of one sample and ALL heads.  g_sym[b,i,:,:] is then one contiguous run of L * H floats per row,
// and the column gather g_sym[b,j,i0:i0+TI,:] is a run of TI * H floats per j (a lone row would read H floats at a stride of
// L * H): phase A stages the half-sum of both in LDS as [ii][h][j], rows padded to an odd length so that the h-fastest writes
// and the j-fastest reads are both free of bank conflicts.  TI is the largest of 16, 8, 4, 2, 1 whose stage fits 64 KB; a
// shape whose single row does not fit (H * L > 16128) reads g_sym from memory in phase B instead (SYM_LDS = false).
// Phase B, a wave per (ii, h) row: the maximum, then the normaliser and sum p dp in fp64 (as in dist_att_bwd_kernel), then
// ds; the logits are read three times and dp twice, the repeats from cache.  No atomics, a fixed order: the same bits run to run.
// ================================================================================================
static inline int tsb_row_ld(int L) { return L | 1; }

template <bool SYM_LDS>
__global__ __launch_bounds__(256) void tied_softmax_bwd_kernel(const float* __restrict__ logits, const float* __restrict__ dp,
                                                               const float* __restrict__ g_sym, float* __restrict__ ds,
                                                               h16_t* __restrict__ p16, h16_t* __restrict__ ds16, int64_t ld,
                                                               int H, int L, int TI, int tiles) {
  extern __shared__ float tsb_sm[];  // [TI][H][L | 1]: the symmetrised map's half-sum (SYM_LDS with g_sym only)
  const int b = blockIdx.x / tiles, i0 = (blockIdx.x - b * tiles) * TI;
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const int nrow = min(TI, L - i0);
  const int Lo = L | 1;
  const int64_t LH = (int64_t)L * H;
  const float* gb = g_sym ? g_sym + (int64_t)b * L * LH : nullptr;
  if (SYM_LDS && gb) {
    // ---- phase A.  The row term: element e = (j, h) of row i0 + ii, contiguous in memory.
    for (int ii = 0; ii < nrow; ++ii) {
      const float* src = gb + (int64_t)(i0 + ii) * LH;
      float* dst = tsb_sm + (int64_t)ii * H * Lo;
      for (int e = t; e < L * H; e += 256) {
        const int j = e / H, h = e - j * H;
        dst[h * Lo + j] = src[e];
      }
    }
    __syncthreads();
    // The column term: element e = (j, ii, h), a run of nrow * H floats per j.  Each LDS word is touched by one thread.
    const int run = nrow * H;
    for (int e = t; e < L * run; e += 256) {
      const int j = e / run, r = e - j * run, ii = r / H, h = r - ii * H;
      float* d = tsb_sm + ((int64_t)ii * H + h) * Lo + j;
      *d = 0.5f * (*d + gb[(int64_t)j * LH + (int64_t)i0 * H + r]);
    }
    __syncthreads();
  }
  // ---- phase B (a lane takes the entries j = lane + 64 m)
  for (int r = wv; r < nrow * H; r += 4) {
    const int ii = r / H, h = r - ii * H, i = i0 + ii;
    const int64_t row = (((int64_t)b * H + h) * L + i) * L;  // element [b, h, i, 0] of logits, dp and ds
    const float* lg = logits + row;
    const float* dr = dp + row;
    const float* sy = tsb_sm + (int64_t)r * Lo;
    auto dp_at = [&](int j) -> float {
      if (!gb) return dr[j];
      if (SYM_LDS) return dr[j] + sy[j];
      return dr[j] + 0.5f * (gb[((int64_t)i * L + j) * H + h] + gb[((int64_t)j * L + i) * H + h]);
    };
    float mx = -INFINITY;
    for (int j = lane; j < L; j += 64) mx = fmaxf(mx, lg[j]);
    mx = wave_max(mx);
    double s = 0.0, dot = 0.0;
    for (int j = lane; j < L; j += 64) {
      const double ex = (double)expf(lg[j] - mx);
      s += ex;
      dot = fma(ex, (double)dp_at(j), dot);
    }
    const double inv = 1.0 / wave_sum_f64(s);
    dot = wave_sum_f64(dot) * inv;
    const int64_t row16 = (((int64_t)b * H + h) * L + i) * ld;
    for (int j = lane; j < L; j += 64) {
      const double p = (double)expf(lg[j] - mx) * inv;
      const float dsv = (float)(p * ((double)dp_at(j) - dot));
      ds[row + j] = dsv;
      if (p16) p16[row16 + j] = f2h((float)p);
      if (ds16) ds16[row16 + j] = f2h(dsv);
    }
    for (int64_t j = L + lane; j < ld; j += 64) {  // the pad columns of the 16-bit copies
      if (p16) p16[row16 + j] = 0;
      if (ds16) ds16[row16 + j] = 0;
    }
  }
}

// include/rfmi.h: rf_tied_softmax_bwd
extern "C" int rf_tied_softmax_bwd(const float* logits, const float* dp, const float* g_sym, float* ds, void* p_h16, void* ds_h16,
                                   int64_t ld, int B, int H, int L, void* stream) {
  if (!logits || !dp || !ds || B <= 0 || H <= 0 || L <= 0) return RF_EINVAL;
  if ((int64_t)L * H > 0x7fffffff / 16) return RF_EINVAL;
  if (p_h16 || ds_h16) {
    if (ld < L) return RF_EINVAL;
    if (ld % 8) return RF_EALIGN;
  }
  const int64_t row_bytes = (int64_t)H * tsb_row_ld(L) * sizeof(float);
  int TI = 16;
  while (TI > 1 && TI * row_bytes > 64 * 1024) TI >>= 1;
  if (!g_sym) TI = L >= 256 ? 4 : 16;  // nothing is staged: rows per block for the launch shape only
  const bool stage = g_sym && TI * row_bytes <= 64 * 1024;
  const int tiles = (L + TI - 1) / TI;
  if ((int64_t)B * tiles > 0x7fffffff) return RF_EINVAL;
  const size_t lds = stage ? (size_t)(TI * row_bytes) : 0;
  hipStream_t s = (hipStream_t)stream;
  if (stage)
    hipLaunchKernelGGL(tied_softmax_bwd_kernel<true>, dim3(B * tiles), dim3(256), lds, s, logits, dp, g_sym, ds, (h16_t*)p_h16,
                       (h16_t*)ds_h16, ld, H, L, TI, tiles);
  else
    hipLaunchKernelGGL(tied_softmax_bwd_kernel<false>, dim3(B * tiles), dim3(256), 0, s, logits, dp, g_sym, ds, (h16_t*)p_h16,
                       (h16_t*)ds_h16, ld, H, L, TI, tiles);
  return rf_launch_status();
}

// ================================================================================================
// rf_scale_rows_bwd: backward of rf_scale_rows (y[r, :] = alpha w[r] x[r, :]) over rows r = (t, h) of D columns: row (t, h)
// of a tensor starts at t * ld + h * hs, w and dw hold one fp32 per row, contiguous.
//   dx[r, :] = alpha w[r] gy[r, :]      dw[r] = alpha sum_c gy[r, c] x[r, c]
// G lanes share a row (G = 8, 16 or 32 by D); the sum runs in fp64 and meets in a shuffle butterfly: a fixed order, no atomics.
// ================================================================================================
template <int G>
__global__ __launch_bounds__(256) void scale_rows_bwd_kernel(const void* x, int x_dt, int64_t x_ld, int64_t x_hs, const void* gy,
                                                             int gy_dt, int64_t gy_ld, int64_t gy_hs, const float* __restrict__ w,
                                                             float alpha, void* dx, int dx_dt, int64_t dx_ld, int64_t dx_hs,
                                                             float* __restrict__ dw, int64_t rows, int H, int D) {
  const int64_t r = (int64_t)blockIdx.x * (256 / G) + threadIdx.x / G;
  const int cl = threadIdx.x % G;
  const bool ok = r < rows;  // (no early return: the shuffles below run with every lane)
  double a = 0.0;
  if (ok) {
    const int64_t tk = r / H;
    const int h = (int)(r - tk * H);
    const int64_t xo = tk * x_ld + h * x_hs, go = tk * gy_ld + h * gy_hs, dxo = tk * dx_ld + h * dx_hs;
    const double aw = (double)alpha * (double)w[r];
    for (int c = cl; c < D; c += G) {
      const float g = ld(gy, gy_dt, go + c);
      a = fma((double)g, (double)ld(x, x_dt, xo + c), a);
      if (dx) st(dx, dx_dt, dxo + c, (float)(aw * (double)g));
    }
  }
#pragma unroll
  for (int o = G / 2; o > 0; o >>= 1) a += __shfl_xor(a, o, 64);
  if (ok && cl == 0 && dw) dw[r] = (float)((double)alpha * a);
}

// include/rfmi.h: rf_scale_rows_bwd
extern "C" int rf_scale_rows_bwd(const void* x, int x_dtype, int64_t x_ld, int64_t x_hs, const void* gy, int gy_dtype, int64_t gy_ld,
                                 int64_t gy_hs, const float* w, float alpha, void* dx, int dx_dtype, int64_t dx_ld, int64_t dx_hs,
                                 float* dw, int64_t tokens, int H, int D, void* stream) {
  RF_CHECK_DT(x_dtype);
  RF_CHECK_DT(gy_dtype);
  if (dx) RF_CHECK_DT(dx_dtype);
  if (!x || !gy || !w || (!dx && !dw) || tokens <= 0 || H <= 0 || D <= 0) return RF_EINVAL;
  if (x_ld < 0 || x_hs < 0 || gy_ld < 0 || gy_hs < 0 || dx_ld < 0 || dx_hs < 0) return RF_EINVAL;
  if (tokens > (int64_t)0x7fffffff * 8 / H) return RF_EINVAL;
  const int64_t rows = tokens * H;
  hipStream_t s = (hipStream_t)stream;
#define SRB_LAUNCH(G_)                                                                                                            \
  hipLaunchKernelGGL(scale_rows_bwd_kernel<G_>, dim3(cdiv(rows, 256 / G_)), dim3(256), 0, s, x, x_dtype, x_ld, x_hs, gy, gy_dtype, \
                     gy_ld, gy_hs, w, alpha, dx, dx_dtype, dx_ld, dx_hs, dw, rows, H, D)
  if (D >= 32)
    SRB_LAUNCH(32);
  else if (D >= 16)
    SRB_LAUNCH(16);
  else
    SRB_LAUNCH(8);
#undef SRB_LAUNCH
  return rf_launch_status();
}

// ================================================================================================
// rf_pair_softmax_bwd: backward of the batched per-(layer, head) softmax of MsaUpdateWithPair's shared front (model.py:
// pair_to_att; ops.hip: softmax_batched_kernel).  The logits live in [B, L, L, NZ], map z = layer * H + head innermost, and the
// softmax of map z runs over j at a stride of NZ floats.  A block owns one (b, i): the NZ rows of that pair row are ONE contiguous
// slab of L * NZ floats, on the way in (logits) and on the way out (dz).
//   phase A  the slab is read with consecutive lanes on consecutive floats and laid down in LDS as [z][j], rows an odd number
//            of floats apart
//   phase B  a wave per map z, a lane on the entries j = lane + 64 m: the maximum, then the normaliser and sum_j p datt in fp64 (as
//            in dist_att_bwd_kernel and tied_softmax_bwd_kernel), then dz = p (datt - sum p datt), which replaces the logit in LDS;
//            the datt row [z, b, i, :] is read along j, twice (the second time from cache)
//   phase C  the slab of dz leaves as it came, consecutive lanes on consecutive floats, and so does the 16-bit copy with its
//            nz_pad columns per (i, j), zeros in the columns [NZ, nz_pad)
// No atomics and a fixed order: the same bits run to run.  L == 1: p = 1 and dz = datt - datt = 0 exactly.
// ================================================================================================
static inline int psb_row_ld(int L) { return L | 1; }

__global__ __launch_bounds__(256) void pair_softmax_bwd_kernel(const float* __restrict__ logits, const float* __restrict__ datt,
                                                               int64_t datt_ld, float* __restrict__ dz, h16_t* __restrict__ dz16,
                                                               int nz_pad, int B, int L, int NZ) {
  extern __shared__ float psb_sm[];  // [NZ][L | 1]: logits, then dz
  const int bi = blockIdx.x, b = bi / L, i = bi - b * L;
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const int Lo = L | 1;
  const int n = L * NZ;
  const int64_t slab = (int64_t)bi * n;
  // ---- phase A
  for (int e = t; e < n; e += 256) {
    const int j = e / NZ, z = e - j * NZ;
    psb_sm[z * Lo + j] = logits[slab + e];
  }
  __syncthreads();
  // ---- phase B
  for (int z = wv; z < NZ; z += 4) {
    float* ps = psb_sm + z * Lo;
    const float* dr = datt + (((int64_t)z * B + b) * L + i) * datt_ld;
    float mx = -INFINITY;
    for (int j = lane; j < L; j += 64) mx = fmaxf(mx, ps[j]);
    mx = wave_max(mx);
    double s = 0.0, dot = 0.0;
    for (int j = lane; j < L; j += 64) {
      const double ex = (double)expf(ps[j] - mx);
      s += ex;
      dot = fma(ex, (double)dr[j], dot);
    }
    const double inv = 1.0 / wave_sum_f64(s);
    dot = wave_sum_f64(dot) * inv;
    for (int j = lane; j < L; j += 64) {
      const double p = (double)expf(ps[j] - mx) * inv;
      ps[j] = (float)(p * ((double)dr[j] - dot));
    }
  }
  __syncthreads();
  // ---- phase C
  for (int e = t; e < n; e += 256) {
    const int j = e / NZ, z = e - j * NZ;
    dz[slab + e] = psb_sm[z * Lo + j];
  }
  if (dz16) {
    const int n16 = L * nz_pad;
    h16_t* out = dz16 + (int64_t)bi * n16;
    for (int e = t; e < n16; e += 256) {
      const int j = e / nz_pad, z = e - j * nz_pad;
      out[e] = z < NZ ? f2h(psb_sm[z * Lo + j]) : (h16_t)0;
    }
  }
}

// include/rfmi.h: rf_pair_softmax_bwd
extern "C" int rf_pair_softmax_bwd(const float* logits, const float* datt, int64_t datt_ld, float* dz, void* dz_h16, int nz_pad,
                                   int B, int L, int NZ, void* stream) {
  if (!logits || !datt || !dz || B <= 0 || L <= 0 || NZ <= 0 || datt_ld < L) return RF_EINVAL;
  if (dz_h16 && (nz_pad < NZ || nz_pad % 8)) return RF_EINVAL;
  if ((int64_t)B * L > 0x7fffffff) return RF_EINVAL;
  const int64_t lds = (int64_t)NZ * psb_row_ld(L) * (int64_t)sizeof(float);
  if (lds > 160 * 1024 || (dz_h16 && (int64_t)L * nz_pad > 0x7fffffff)) return RF_EINVAL;
  if (lds > 64 * 1024) {
    const int rc = rf_enable_big_lds<pair_softmax_bwd_kernel>();
    if (rc) return rc;
  }
  hipLaunchKernelGGL(pair_softmax_bwd_kernel, dim3(B * L), dim3(256), (size_t)lds, (hipStream_t)stream, logits, datt, datt_ld, dz,
                     (h16_t*)dz_h16, nz_pad, B, L, NZ);
  return rf_launch_status();
}

// ================================================================================================
// rf_sym_layernorm_bwd: backward of z = rf_sym_layernorm(pair) . w^T, the shared front of MsaUpdateWithPair (symmetrise ->
// LayerNorm without affine -> the folded projection W * gamma, model.py: pair_to_att).  With s = (pair_ij + pair_ji) / 2 -- the
// same numbers for (i, j) and (j, i), so one xhat and one rstd serve both -- and g = (dz_ij + dz_ji) . w:
//   dpair_ij = dpair_ji = rstd / 2 * (g - mean g - xhat * mean(g xhat))          (the diagonal: the same formula)
// A wave takes one unordered pair i <= j: both pair rows and both dz rows are read once, g is formed in registers from w in LDS
// (NZ fp32 FMAs per element; lane z holds dz_ij[z] + dz_ji[z] and hands it round by a shuffle), the statistics are recomputed two-pass
// in fp32 with the forward's expressions, the two means are fp64 sums, and both output rows are written: no [B, L, L, D]
// intermediate, each element of pair read once and each element of dpair written once, both as 16-byte pieces per lane.
// The pairs are numbered without a square root: row r and row L - 1 - r of the upper triangle hold L + 1 pairs together, so item
// (r, c), r < ceil(L / 2), c <= L, is (r, r + c) for c < L - r and (L - 1 - r, c - 1) past it (the middle row of an odd L once).
// NV = 16-byte pieces per lane (D <= 256 NV); WLDS: w fits 64 KB of LDS, else it is read from memory (cache) in place.
// ================================================================================================
template <int NV, bool WLDS>
__global__ __launch_bounds__(256) void sym_layernorm_bwd_kernel(const float* __restrict__ pair, const float* __restrict__ dz,
                                                                const float* __restrict__ w, float* __restrict__ dpair, int L,
                                                                int D, int NZ, float eps, int64_t items, int R) {
  extern __shared__ float slb_sm[];  // WLDS: w [NZ][D]
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  if (WLDS) {
    for (int e = t; e < NZ * D; e += 256) slb_sm[e] = w[e];
    __syncthreads();
  }
  const int nch = D >> 2;
  int c4[NV];  // this lane's pieces; a lane past the row computes on the row's last piece and writes nothing
  bool ok[NV];
#pragma unroll
  for (int v = 0; v < NV; ++v) {
    ok[v] = lane + 64 * v < nch;
    c4[v] = ok[v] ? lane + 64 * v : nch - 1;
  }
  const float invD = 1.f / (float)D;
  for (int64_t it = (int64_t)blockIdx.x * 4 + wv; it < items; it += (int64_t)gridDim.x * 4) {  // (wave-uniform)
    const int64_t br = it / (L + 1);
    const int c = (int)(it - br * (L + 1));
    const int b = (int)(br / R), r = (int)(br - (int64_t)b * R);
    int i, j;
    if (c < L - r) {
      i = r;
      j = r + c;
    } else {
      i = L - 1 - r;
      if (i == r) continue;
      j = c - 1;
    }
    const int64_t rij = ((int64_t)b * L + i) * L + j, rji = ((int64_t)b * L + j) * L + i;
    const float4* pa = (const float4*)(pair + rij * D);
    const float4* pb = (const float4*)(pair + rji * D);
    const float gzl = lane < NZ ? dz[rij * NZ + lane] + dz[rji * NZ + lane] : 0.f;
    float4 s[NV];
    float sum = 0.f;
#pragma unroll
    for (int v = 0; v < NV; ++v) {
      const float4 a = pa[c4[v]], bb = pb[c4[v]];
      s[v] = make_float4(0.5f * (a.x + bb.x), 0.5f * (a.y + bb.y), 0.5f * (a.z + bb.z), 0.5f * (a.w + bb.w));
      if (ok[v]) sum += (s[v].x + s[v].y) + (s[v].z + s[v].w);
    }
    const float mean = wave_sum(sum) * invD;
    float q = 0.f;
#pragma unroll
    for (int v = 0; v < NV; ++v) {
      s[v].x -= mean; s[v].y -= mean; s[v].z -= mean; s[v].w -= mean;
      if (ok[v]) q += (s[v].x * s[v].x + s[v].y * s[v].y) + (s[v].z * s[v].z + s[v].w * s[v].w);
    }
    const float rstd = rsqrtf(wave_sum(q) * invD + eps);
    float4 g[NV];
#pragma unroll
    for (int v = 0; v < NV; ++v) g[v] = make_float4(0.f, 0.f, 0.f, 0.f);
    const float* wp = WLDS ? slb_sm : w;
#pragma unroll 4
    for (int z = 0; z < NZ; ++z) {
      const float gz = __shfl(gzl, z, 64);
#pragma unroll
      for (int v = 0; v < NV; ++v) {
        const float4 w4 = *(const float4*)(wp + (int64_t)z * D + 4 * c4[v]);
        g[v].x = fmaf(gz, w4.x, g[v].x); g[v].y = fmaf(gz, w4.y, g[v].y);
        g[v].z = fmaf(gz, w4.z, g[v].z); g[v].w = fmaf(gz, w4.w, g[v].w);
      }
    }
    double m1 = 0.0, m2 = 0.0;
#pragma unroll
    for (int v = 0; v < NV; ++v) {
      s[v].x *= rstd; s[v].y *= rstd; s[v].z *= rstd; s[v].w *= rstd;  // xhat
      if (ok[v]) {
        m1 += ((double)g[v].x + (double)g[v].y) + ((double)g[v].z + (double)g[v].w);
        m2 += ((double)g[v].x * (double)s[v].x + (double)g[v].y * (double)s[v].y) +
              ((double)g[v].z * (double)s[v].z + (double)g[v].w * (double)s[v].w);
      }
    }
    const float mg = (float)(wave_sum_f64(m1) / (double)D), mgx = (float)(wave_sum_f64(m2) / (double)D);
    const float hr = 0.5f * rstd;
    float4* oa = (float4*)(dpair + rij * D);
    float4* ob = (float4*)(dpair + rji * D);
#pragma unroll
    for (int v = 0; v < NV; ++v) {
      if (ok[v]) {
        const float4 o = make_float4(hr * (g[v].x - mg - s[v].x * mgx), hr * (g[v].y - mg - s[v].y * mgx),
                                     hr * (g[v].z - mg - s[v].z * mgx), hr * (g[v].w - mg - s[v].w * mgx));
        oa[c4[v]] = o;
        if (i != j) ob[c4[v]] = o;
      }
    }
  }
}

// include/rfmi.h: rf_sym_layernorm_bwd
extern "C" int rf_sym_layernorm_bwd(const float* pair, const float* dz, const float* w, float* dpair, int B, int L, int D, int NZ,
                                    float eps, void* stream) {
  if (!pair || !dz || !w || !dpair || B <= 0 || L <= 0 || D <= 0 || NZ <= 0) return RF_EINVAL;
  if (D % 4 || D > 1024 || NZ > 64) return RF_EINVAL;
  if (((uintptr_t)pair % 16) || ((uintptr_t)dpair % 16) || ((uintptr_t)w % 16)) return RF_EALIGN;
  const int R = (L + 1) / 2;
  if ((int64_t)B * R > 0x7fffffff) return RF_EINVAL;
  const int64_t items = (int64_t)B * R * (L + 1);
  const size_t wbytes = (size_t)NZ * D * sizeof(float);
  const bool wlds = wbytes <= 64 * 1024;
  const dim3 grid((unsigned)(items < 4 * 2048 ? cdiv(items, 4) : 2048));
  hipStream_t s = (hipStream_t)stream;
#define SLB_LAUNCH(NV_)                                                                                                            \
  do {                                                                                                                             \
    if (wlds)                                                                                                                      \
      hipLaunchKernelGGL((sym_layernorm_bwd_kernel<NV_, true>), grid, dim3(256), wbytes, s, pair, dz, w, dpair, L, D, NZ, eps,     \
                         items, R);                                                                                                \
    else                                                                                                                           \
      hipLaunchKernelGGL((sym_layernorm_bwd_kernel<NV_, false>), grid, dim3(256), 0, s, pair, dz, w, dpair, L, D, NZ, eps, items, \
                         R);                                                                                                       \
  } while (0)
  if (D <= 256)
    SLB_LAUNCH(1);
  else if (D <= 512)
    SLB_LAUNCH(2);
  else
    SLB_LAUNCH(4);
#undef SLB_LAUNCH
  return rf_launch_status();
}

// ================================================================================================
// Backward of MsaEmbedding and PairEmbedding (model.py; rf.py:106-181): the gradient of an embedding table (a reduction of the
// output gradient keyed by the token index, with the forward's dropout mask replayed) and the sums of a pair-shaped gradient
// over each of its two picture axes.  Both read the gradient once, accumulate in fp64 and write fp64 partials to a
// caller-owned workspace, which one launch of ordered_sum_f64_kernel adds in a fixed order and rounds once: no atomics.
// ================================================================================================
// out[x] = (float) sum_{k = 0 .. S-1} part[k * stride + x] for up to four independent segments laid end to end
struct SumSeg {
  const double* part;
  float* out;
  int64_t n, stride;
  int S;
};
struct SumSegs {
  SumSeg s[4];
};

__global__ __launch_bounds__(256) void ordered_sum_f64_kernel(SumSegs a, int64_t total) {
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
    const double* part = nullptr;
    float* out = nullptr;
    int64_t x = e, stride = 0;
    int S = 0;
    bool found = false;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (!found && x < a.s[k].n) {
        part = a.s[k].part + x, out = a.s[k].out + x, stride = a.s[k].stride, S = a.s[k].S;
        found = true;
      }
      if (!found) x -= a.s[k].n;
    }
    if (!found) continue;
    double s = 0.0;
#pragma unroll 8
    for (int k = 0; k < S; ++k) s += part[(int64_t)k * stride];
    *out = (float)s;
  }
}

static inline void launch_ordered_sum(const SumSegs& segs, hipStream_t s) {
  int64_t total = 0;
  for (int k = 0; k < 4; ++k) total += segs.s[k].n;
  hipLaunchKernelGGL(ordered_sum_f64_kernel, dim3(min(cdiv(total, 256), 16384u)), dim3(256), 0, s, segs, total);
}

// ---- rf_embedding_bwd -----------------------------------------------------------------------------------------------------------
// A wave owns EMB_ROWS consecutive rows and 64 channels (one per lane); a block is W = 4, 2 or 1 such waves on consecutive row
// ranges.  Each wave keeps fp64 sums [V][64] of its own in LDS, every entry touched by its one lane only (no synchronisation
// while accumulating), and the two query-encoding sums in registers; the block adds its waves' sums in wave order and writes
// one partial [V + 2][D-tile] per block.  W is the largest count whose sums fit 64 KB of LDS.
#define EMB_ROWS 256
#define EMB_LDS_LIMIT (64 * 1024)

static inline int emb_waves(int V) {
  for (int W = 4; W >= 1; W >>= 1)
    if ((size_t)W * (V + 2) * 64 * sizeof(double) <= EMB_LDS_LIMIT) return W;
  return 0;
}

template <bool DROP>
__global__ __launch_bounds__(256) void embedding_bwd_kernel(const int64_t* __restrict__ idx, const float* __restrict__ g,
                                                            double* __restrict__ part, int64_t rows, int D, int V, int N, int L,
                                                            unsigned thresh, float inv_keep, uint64_t seed, uint64_t offset) {
  extern __shared__ double emb_acc[];  // [W][V + 2][64]
  const int W = blockDim.x >> 6, w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int c = blockIdx.y * 64 + lane;
  const int T = V + 2;
  double* mine = emb_acc + (size_t)w * T * 64 + lane;
  for (int t = 0; t < T; ++t) mine[t * 64] = 0.0;
  const int64_t r0 = ((int64_t)blockIdx.x * W + w) * EMB_ROWS;
  const int64_t r1 = r0 + EMB_ROWS < rows ? r0 + EMB_ROWS : rows;
  if (c < D && r0 < r1) {
    int l = (int)(r0 % L), n = (int)((r0 / L) % N);  // the row's position (n, l) of [.., N, L], stepped with the row
    double q0 = 0.0, q1 = 0.0;
    for (int64_t r = r0; r < r1; r += 8) {
      float v[8];
      int64_t t[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const bool ok = r + u < r1;
        t[u] = ok ? idx[r + u] : -1;
        v[u] = ok ? g[(r + u) * D + c] : 0.f;
      }
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        if (r + u < r1) {
          if (n == 0)
            q0 += (double)v[u];
          else
            q1 += (double)v[u];
          if (++l == L) {
            l = 0;
            if (++n == N) n = 0;
          }
          if ((uint64_t)t[u] < (uint64_t)V) {  // (an index outside the table contributes nothing)
            float m = v[u];
            if (DROP) m = dropout_keep(seed, offset, (r + u) * D + c, thresh) ? m * inv_keep : 0.f;  // rf_dropout's own product
            mine[t[u] * 64] += (double)m;
          }
        }
      }
    }
    mine[V * 64] = q0;
    mine[(V + 1) * 64] = q1;
  }
  __syncthreads();
  if (c < D)
    for (int t = w; t < T; t += W) {
      double s = 0.0;
      for (int k = 0; k < W; ++k) s += emb_acc[((size_t)k * T + t) * 64 + lane];
      part[((int64_t)blockIdx.x * T + t) * D + c] = s;
    }
}

static inline int64_t emb_blocks(int64_t rows, int W) { return (rows + (int64_t)W * EMB_ROWS - 1) / ((int64_t)W * EMB_ROWS); }

extern "C" int64_t rf_embedding_bwd_ws_bytes(int64_t rows, int D, int V) {
  if (rows <= 0 || D <= 0 || V <= 0) return 0;
  const int W = emb_waves(V);
  if (!W) return 0;
  return emb_blocks(rows, W) * (V + 2) * D * (int64_t)sizeof(double);
}

// include/rfmi.h: rf_embedding_bwd
extern "C" int rf_embedding_bwd(const int64_t* idx, const float* g, float* dtable, float* dq, int64_t rows, int D, int V, int N,
                                int L, float p, uint64_t seed, uint64_t offset, void* workspace, int64_t ws_bytes, void* stream) {
  if (!idx || !g || !dtable || rows <= 0 || D <= 0 || V <= 0 || N <= 0 || L <= 0) return RF_EINVAL;
  if (!(p >= 0.f) || !(p < 1.f)) return RF_EINVAL;
  const int W = emb_waves(V);
  if (!W) return RF_EINVAL;
  const int64_t nblk = emb_blocks(rows, W);
  if (nblk > 0x7fffffff || cdiv(D, 64) > 65535u) return RF_EINVAL;
  if (!workspace || ((uintptr_t)workspace % 8) || ws_bytes < rf_embedding_bwd_ws_bytes(rows, D, V)) return RF_EINVAL;
  double* part = (double*)workspace;
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((unsigned)nblk, cdiv(D, 64));
  const size_t lds = (size_t)W * (V + 2) * 64 * sizeof(double);
  if (p > 0.f)
    hipLaunchKernelGGL(embedding_bwd_kernel<true>, grid, dim3(64 * W), lds, s, idx, g, part, rows, D, V, N, L,
                       dropout_threshold(p), 1.f / (1.f - p), seed, offset);
  else
    hipLaunchKernelGGL(embedding_bwd_kernel<false>, grid, dim3(64 * W), lds, s, idx, g, part, rows, D, V, N, L, 0u, 1.f, seed,
                       offset);
  const int64_t T = V + 2;
  SumSegs segs = {};
  segs.s[0] = {part, dtable, (int64_t)V * D, T * D, (int)nblk};
  if (dq) segs.s[1] = {part + (int64_t)V * D, dq, (int64_t)2 * D, T * D, (int)nblk};
  launch_ordered_sum(segs, s);
  return rf_launch_status();
}

// ---- rf_pair_axis_sums ----------------------------------------------------------------------------------------------------------
// A block takes a PAS_TI x PAS_TJ tile (i, j) of one sample's picture and 64 channels (one per lane).  Wave w walks the tile's
// columns j = w, w + 4, ..: per column the PAS_TI rows are loaded together, their sum is the column's partial for this row tile
// (written at once), and each adds to the row's fp64 register sum and, times the separation feature, to dsep's.  The four waves'
// row sums meet in LDS and are added in wave order into the row partial of this column tile; so do their dsep and dbias sums.
#define PAS_TI 16
#define PAS_TJ 64

__global__ __launch_bounds__(256) void pair_axis_sums_kernel(const float* __restrict__ g, const int64_t* __restrict__ aa_idx,
                                                             double* __restrict__ colp, double* __restrict__ rowp,
                                                             double* __restrict__ sbp, int B, int L, int D, int nIt, int nJt) {
  __shared__ float sep[PAS_TI][PAS_TJ];
  __shared__ double red[4][PAS_TI][64];
  __shared__ double red2[4][2][64];
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int c = blockIdx.y * 64 + lane;
  const int bid = blockIdx.x;
  const int jt = bid % nJt, it = (bid / nJt) % nIt, b = bid / (nJt * nIt);
  const int i0 = it * PAS_TI, j0 = jt * PAS_TJ;
  for (int t = threadIdx.x; t < PAS_TI * PAS_TJ; t += 256) {
    const int ii = t / PAS_TJ, jj = t % PAS_TJ;
    float sv = 0.f;
    if (i0 + ii < L && j0 + jj < L) {  // the forward's own expression (pair_embed_kernel, csrc/ops.hip)
      const int64_t a = aa_idx[(int64_t)b * L + i0 + ii], e = aa_idx[(int64_t)b * L + j0 + jj];
      const int64_t dd = a > e ? a - e : e - a;
      sv = logf((float)(dd + 1));
    }
    sep[ii][jj] = sv;
  }
  __syncthreads();
  const bool on = c < D;
  double racc[PAS_TI];
#pragma unroll
  for (int ii = 0; ii < PAS_TI; ++ii) racc[ii] = 0.0;
  double ds = 0.0;
  for (int jj = w; jj < PAS_TJ; jj += 4) {
    const int j = j0 + jj;
    if (j >= L) break;
    float v[PAS_TI];
#pragma unroll
    for (int ii = 0; ii < PAS_TI; ++ii)
      v[ii] = (on && i0 + ii < L) ? g[(((int64_t)b * L + i0 + ii) * L + j) * D + c] : 0.f;
    double cacc = 0.0;
#pragma unroll
    for (int ii = 0; ii < PAS_TI; ++ii) {
      const double x = (double)v[ii];
      cacc += x;
      racc[ii] += x;
      ds += x * (double)sep[ii][jj];
    }
    if (on) colp[(((int64_t)it * B + b) * L + j) * D + c] = cacc;
  }
  double db = 0.0;
#pragma unroll
  for (int ii = 0; ii < PAS_TI; ++ii) {
    red[w][ii][lane] = racc[ii];
    db += racc[ii];
  }
  red2[w][0][lane] = ds;
  red2[w][1][lane] = db;
  __syncthreads();
  if (!on) return;
  for (int ii = w; ii < PAS_TI; ii += 4)
    if (i0 + ii < L)
      rowp[(((int64_t)jt * B + b) * L + i0 + ii) * D + c] = ((red[0][ii][lane] + red[1][ii][lane]) + red[2][ii][lane]) + red[3][ii][lane];
  if (w < 2) sbp[((int64_t)bid * 2 + w) * D + c] = ((red2[0][w][lane] + red2[1][w][lane]) + red2[2][w][lane]) + red2[3][w][lane];
}

extern "C" int64_t rf_pair_axis_sums_ws_bytes(int B, int L, int D) {
  if (B <= 0 || L <= 0 || D <= 0) return 0;
  const int64_t nIt = cdiv(L, PAS_TI), nJt = cdiv(L, PAS_TJ);
  return ((nIt + nJt) * B * L + 2 * (int64_t)B * nIt * nJt) * D * (int64_t)sizeof(double);
}

// include/rfmi.h: rf_pair_axis_sums
extern "C" int rf_pair_axis_sums(const float* g, const int64_t* aa_idx, float* rows, float* cols, float* dsep, float* dbias, int B,
                                 int L, int D, void* workspace, int64_t ws_bytes, void* stream) {
  if (!g || !aa_idx || !rows || !cols || !dsep || !dbias || B <= 0 || L <= 0 || D <= 0) return RF_EINVAL;
  const int64_t nIt = cdiv(L, PAS_TI), nJt = cdiv(L, PAS_TJ);
  const int64_t nblk = (int64_t)B * nIt * nJt;
  if (nblk > 0x7fffffff || cdiv(D, 64) > 65535u) return RF_EINVAL;
  if (!workspace || ((uintptr_t)workspace % 8) || ws_bytes < rf_pair_axis_sums_ws_bytes(B, L, D)) return RF_EINVAL;
  const int64_t bld = (int64_t)B * L * D;
  double* colp = (double*)workspace;
  double* rowp = colp + nIt * bld;
  double* sbp = rowp + nJt * bld;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(pair_axis_sums_kernel, dim3((unsigned)nblk, cdiv(D, 64)), dim3(256), 0, s, g, aa_idx, colp, rowp, sbp, B, L, D,
                     (int)nIt, (int)nJt);
  SumSegs segs = {};
  segs.s[0] = {colp, cols, bld, bld, (int)nIt};
  segs.s[1] = {rowp, rows, bld, bld, (int)nJt};
  segs.s[2] = {sbp, dsep, (int64_t)D, (int64_t)2 * D, (int)nblk};
  segs.s[3] = {sbp + D, dbias, (int64_t)D, (int64_t)2 * D, (int)nblk};
  launch_ordered_sum(segs, s);
  return rf_launch_status();
}
