/* rfmi.h -- C ABI of librfmi.so, the MI355X (gfx950) RoseTTAFold forward-path kernels.
 *
 * The reference (dohlee/rosettafold-pytorch) has no FFI / plugin interface: its only boundary
 * is the Python nn.Module call surface.  This header is the boundary the
 * build adds underneath that surface: one `extern "C"` entry point per op group of the
 * forward path, each citing the reference lines whose arithmetic it replaces.  The Python
 * host (rosettafold-pytorch_amd/) binds these with ctypes; INTEGRATION.md shows the stub.
 *
 * Conventions (all entry points):
 *   - every pointer is a DEVICE pointer; the caller allocates every output and workspace;
 *   - kernels are launched on `stream` (a hipStream_t passed as void*), never allocate,
 *     never synchronise, keep no global state: re-entrant;
 *   - return value: 0 = launched; >0 = hipError_t from the launch; <0 = argument rejected
 *     (RF_EINVAL...) and nothing was launched;
 *   - dtype codes: RF_F32 = 0, RF_BF16 = 1, RF_F16 = 2.  "T" below = activation dtype chosen by the caller.
 *     RF_F32X3 = 3 is an operand code of rf_gemm_desc.ab_dtype alone (fp32 operands, split-bf16 contraction); every other
 *     dtype argument of every entry point rejects it with RF_EINVAL.
 *   - the kernel sources are built twice: librfmi.so computes its 16-bit MFMA contractions in bfloat16
 *     (v_mfma_f32_16x16x32_bf16) and accepts {RF_F32, RF_BF16}; librfmi_f16.so computes them in IEEE fp16
 *     (v_mfma_f32_16x16x32_f16: same rate and bytes, 11 significand bits instead of 8, range 65504) and accepts
 *     {RF_F32, RF_F16}.  Both export exactly the symbols declared here; rf_h16_dtype() says which 16-bit code a
 *     loaded library takes, every other 16-bit code is rejected with RF_EINVAL.  Wherever a comment below says
 *     "bf16" for an operand it means "the library's 16-bit type".
 */
#ifndef RFMI_H
#define RFMI_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RF_F32 0
#define RF_BF16 1
#define RF_F16 2
/* rf_gemm_desc.ab_dtype only: A and B are fp32 in memory and each element x is split in the kernel into bf16 pieces
 * hi = bf16(x), lo = bf16(x - hi) (round to nearest even; lo = 0 when hi is not finite, and the two cross products take hi with
 * its non-finite elements zeroed, so inf / NaN enter through hi_a.hi_b alone and propagate as on the exact path).
 * C = hi_a.hi_b + hi_a.lo_b + lo_a.hi_b with fp32 accumulation (v_mfma_f32_16x16x32_bf16, three per product; lo.lo is
 * dropped): the "high" float32 matmul precision of PyTorch.  The same bf16 pieces in both libraries, so librfmi.so and
 * librfmi_f16.so give identical results.  Error bound per element (|x| < 3.39e38, the bf16 range):
 *   |C - C_exact| <= (3 * 2^-16 + K * 2^-23) * sum_k |a_k| |b_k|   (+ the fp32 rounding of alpha / bias / residual)
 * (each dropped piece -- lo.lo, and the rounding of lo on either side -- is at most 2^-16 |a b|; random data sits orders of
 * magnitude below the bound).  Takes and rejects exactly the descriptors of RF_F32. */
#define RF_F32X3 3

#define RF_EINVAL (-1)   /* inconsistent sizes / unsupported combination */
#define RF_EALIGN (-2)   /* pointer or stride not aligned as the kernel needs */

#define RF_ACT_NONE 0
#define RF_ACT_RELU 1
#define RF_ACT_ELU 2
#define RF_ACT_RELU_EPS 3 /* relu(x)+eps for column < act_nvalid (row < -act_nvalid if negative), 0 beyond (FAVOR+ ReLU features) */
#define RF_ACT_LEAKY 4    /* LeakyReLU(0.01), rf_layernorm only */
#define RF_ACT_BLOCK_LN32 5 /* rf_gemm, bf16 path, 256x256 tiles: LayerNorm over every aligned 32x32 block of the output
                            * (block (i,j) = rows 32i.., cols 32j..; feature k = 32*(row%32) + col%32) with affine
                            * ln_gamma/ln_beta[1024], ln_eps; ln_out must be NULL.  The outer-product features of
                            * OuterProductMean normalised in the GEMM epilogue (rf.py:416,424-426). */

#define RF_BIAS_NONE 0
#define RF_BIAS_COL 1 /* bias[n] */
#define RF_BIAS_ROW 2 /* bias[m] */

#define RF_AMODE_PLAIN 0
#define RF_AMODE_CONV3X3 1 /* A rows are NHWC pixels, K = 9*C im2col on the fly */

/* Strided / batched / chunked GEMM:  C[z][m][n] = epilogue( alpha * sum_k A[z][m][k] * B[z][n][k] ).
 * Both operands are K-contiguous ("TN"); every contraction of the forward path is phrased
 * this way (nn.Linear rf.py:195-281, the einsums rf.py:254,257,424,592,916, conv2d rf.py:452-457,
 * resnet.py:19-38).  Element offsets (in elements of the operand dtype):
 *   batch z = (z0*nb1 + z1)*nb2 + z2
 *   A(z,m,k) = z0*a_bs[0]+z1*a_bs[1]+z2*a_bs[2] + (m / a_rc)*a_ro + (m % a_rc)*a_ri + (k / kc)*a_ko + (k % kc)
 *   B(z,n,k) = likewise with b_*            (kc = K for a plain contiguous K)
 *   C(z,m,n) = z.c_bs + (m / c_rc)*c_ro + (m % c_rc)*c_ri + (n / c_cc)*c_co + (n % c_cc)
 * a_rc/b_rc/c_rc/c_cc <= 0 mean "no split" (offset = m*..ri, n).
 * RF_AMODE_CONV3X3: A is NHWC [conv_n, conv_h, conv_w, conv_c], m = pixel index, k = tap*C + c
 * (tap = 3*(di+1)+(dj+1)), zero padding, dilation conv_dil; a_* strides are ignored.
 * Non-finite values: the result is NaN wherever the exact product, or the input of the activation, is NaN, in every kernel
 * family and operand type (a Linear does not turn a NaN into -inf, a ReLU does not turn it into 0: RF_ACT_RELU and
 * RF_ACT_RELU_EPS keep NaN like torch.relu); rf_ffn_fused's hidden ReLU follows the same rule.  +-inf leaves with its sign.
 * alpha must be finite and non-zero: RF_EINVAL otherwise, for every ab_dtype (a product scaled by zero is a fill, not a
 * contraction: rf_fill; the 16-bit kernels start their accumulators at bias / alpha).
 */
typedef struct rf_gemm_desc {
  int32_t M, N, K;
  int32_t nb0, nb1, nb2;
  int32_t ab_dtype;  /* the library's 16-bit code (MFMA path), RF_F32 (exact f32 path) or RF_F32X3 (fp32 operands, split-bf16) */
  int32_t c_dtype;   /* RF_BF16 or RF_F32 */
  int32_t kc;
  int32_t a_mode;
  int32_t a_rc, b_rc, c_rc, c_cc;
  int64_t a_bs[3], a_ro, a_ri, a_ko;
  int64_t b_bs[3], b_ro, b_ri, b_ko;
  int64_t c_bs[3], c_ro, c_ri, c_co;
  int32_t conv_n, conv_h, conv_w, conv_c, conv_dil;
  int32_t bias_mode;
  int32_t act;
  int32_t act_nvalid;
  float act_eps;
  float alpha;
  int32_t tile_cfg;  /* 0 = auto; else index into the tile table (tuning/tests) */
  const void* A;
  const void* B;
  void* C;
  const float* bias;     /* fp32 */
  const float* residual; /* fp32, same layout as C; C = residual + epilogue(...) ; may alias C */
  /* optional fused LayerNorm of the result rows (the next sub-layer's pre-norm, rf.py:341 etc.): when ln_out != NULL
   * the kernel also writes ln_out[m, :] = LayerNorm(C[m, :]) * ln_gamma + ln_beta as bf16 [M, N] (row-major).
   * Needs the bf16 path, plain fp32 C, one batch, N <= 384 (a workgroup then owns complete rows). */
  void* ln_out;
  const float* ln_gamma;
  const float* ln_beta;
  float ln_eps;
  int32_t reserved_;
  /* optional row-group scale of the leading output columns, applied to the fp32 accumulators (bias included) before the
   * result is rounded:   C[m][n] *= rs_alpha * rs[(m / rs_rpb) * rs_bstride + (n / rs_cg) * rs_rpb + m % rs_rpb]   for n < rs_ncols.
   * The q | k | v projection of the tied MSA-row attention folds the position weights into q this way (rf.py:252:
   * q * w * d_head^-0.5 with w [B, H, N, L]: rs_rpb = N L, rs_bstride = H N L, rs_cg = d_head, rs_ncols = d_msa), so q is
   * rounded once, after the scaling, and the attention kernels take it as it is.  16-bit path, register-resident-weights
   * kernel only (K = 288 / 384, long M; rs_cg % 16 == 0): RF_EINVAL when rs != NULL and that kernel does not apply. */
  const float* rs;
  int64_t rs_bstride;
  int32_t rs_rpb, rs_cg, rs_ncols;
  float rs_alpha;
} rf_gemm_desc;

int rf_gemm(const rf_gemm_desc* d, void* stream);
/* Introspection for measurement tools: the kernel family the calling thread's last rf_gemm launched (0 exact fp32, 1 generic
 * bf16 tile kernel, 2 conv3x3 implicit GEMM, 3 persistent tile kernel, 4 register-resident-weights skinny-K kernel, 5 split-bf16
 * fp32 kernel (RF_F32X3), -1 none). */
int rf_gemm_last_family(void);

/* LayerNorm over the last dim (nn.LayerNorm, rf.py:323,328,416,435,437,442,443,565,573,580,672,
 * 685,686,758,759,765,771,876,877,883,886,1136; ea/modules.py:553).  rows x D, fp32 statistics. */
int rf_layernorm(const void* x, int x_dtype, int64_t x_ld, void* y, int y_dtype, int64_t y_ld, int64_t rows,
                 int D, const float* gamma, const float* beta, float eps, int groups, int act, void* stream);
/* groups > 1: row r uses gamma/beta[(r % groups)*D ..] (the 8 radial MLPs of one SE(3) layer normalised in one
 * launch, ea/modules.py:265-275); act: RF_ACT_NONE | RF_ACT_RELU | RF_ACT_LEAKY applied after the affine. */

/* y[r, :] = 0.5*(x[b,i,j,:] + x[b,j,i,:]) normalised WITHOUT affine (shared front of the four
 * MsaUpdateWithPairLayer.pair2att of a block: Symmetrization + LayerNorm, rf.py:550-566). */
int rf_sym_layernorm(const float* pair, void* y, int y_dtype, int B, int L, int D, float eps, void* stream);

/* Introspection for tests and measurement tools, like rf_gemm_last_family: the kernel the calling thread's last successful
 * rf_layernorm, rf_sym_layernorm, rf_instnorm_stats, rf_instnorm_apply, rf_axpby or rf_tile_1d_feats launched (-1 none; after
 * a call that returned an error the value is unspecified).  Host-side only, no kernel sees it.
 *    1 / 2    layernorm_rows8 (D = 288 / 384, fp32 in, 16-byte aligned, leading dimensions % 4 == 0)
 *    3 / 4    the same kernels in rf_sym_layernorm
 *    5 / 6    layernorm_vec with 2 / 4 chunks per lane (fp32 in, D % 4 == 0, 128 <= D <= 512 / 512 < D <= 1024, aligned)
 *    7        layernorm_vec_bf16 (16-bit in, D % 8 == 0, 512 < D <= 1024, no activation, aligned)
 *    8 / 9    layernorm_narrow (D = 32 / 64, fp32 in, aligned; takes groups and act)
 *   10 .. 16  the generic one-wave-per-row kernel with 1, 2, 5, 6, 8, 16, 36 values per lane
 *             (D <= 64, 128, 320, 384, 512, 1024, 2304): any dtype, alignment, leading dimension, groups
 *   20 .. 26  the same seven instantiations in rf_sym_layernorm
 *   30 / 31   rf_instnorm_stats: generic (128 pixels per block) / vectorised (16-bit in, C % 8 == 0, aligned; 512 pixels)
 *   32        rf_instnorm_apply: generic (also the centre-only form)
 *   33 / 34   rf_instnorm_apply vectorised, every thread keeping one channel chunk / re-deriving the chunk from the index
 *             (the grid stride is no multiple of C / 8: ceil(HW * (C / 8) / 256) < (C / 8) / gcd(C / 8, 256), small pictures)
 *   40 / 41   rf_axpby scalar / 4 elements per thread (n % 4 == 0, aligned)
 *   42 / 43   rf_tile_1d_feats scalar / 4 channels per thread (P2, c0, feat_ld % 4 == 0, aligned) */
int rf_rowops_last_route(void);

/* Row softmax with strides: for r in [0,rows): y[r*y_rs + c] = softmax_c(scale * x[r*x_rs + c*x_cs]).
 * (rf.py:215,255,569,657,914). */
int rf_softmax(const float* x, int64_t x_rs, int64_t x_cs, void* y, int y_dtype, int64_t y_rs, int64_t rows,
               int cols, float scale, void* stream);

/* nbatch such problems in one launch: problem z reads x + z*x_bs, writes y + z*y_bs (the per-(layer, head) softmaxes of one
 * MsaUpdateWithPair stack, rf.py:569). */
int rf_softmax_batched(const float* x, int64_t x_bs, int64_t x_rs, int64_t x_cs, void* y, int y_dtype, int64_t y_bs,
                       int64_t y_rs, int64_t rows, int cols, float scale, int nbatch, void* stream);

/* Tied-attention softmax (rf.py:255,261-265): logits fp32 [B,H,L,L] -> att T [B,H,L,L] and, when
 * att_sym != NULL, the symmetrised map 0.5*(att+att^T) as fp32 [B,L,L,H] (written with ld sym_ld). */
int rf_tied_softmax(const float* logits, void* att, int att_dtype, float* att_sym, int64_t sym_ld, int B, int H,
                    int L, void* stream);

/* Tied MSA-row attention, logits + softmax in one launch (rf.py:252-255,261-265), bf16 only:
 *   att[b,h,i,:] = softmax_j( sum_{n,d} q[b,n,i,h,d] * k[b,n,j,h,d] )   -> att bf16 [B,H,L,L]
 * q / k element (b,n,l,h,d) at b*b_stride + n*n_stride + l*l_stride + h*d_head + d (q already scaled, rf.py:252);
 * d_head == 32 and L in {64,128,192,256} (RF_EINVAL otherwise: use rf_gemm + rf_tied_softmax).  att_sym as in
 * rf_tied_softmax (may be NULL). */
int rf_tied_logits_softmax(const void* q, const void* k, int64_t b_stride, int64_t n_stride, int64_t l_stride, void* att,
                           float* att_sym, int64_t sym_ld, int B, int H, int N, int L, int d_head, void* stream);

/* Attention . V of the tied attention (rf.py:257-258): out[b,n,i,h,:] = sum_j att[b,h,i,j] v[b,n,h,j,:], bf16.
 * att: [B,H,L,L]; v / out element (b,n,h,l,d) at b*s[0] + n*s[1] + h*s[2] + l*s[3] + d (the 32-wide head slice
 * contiguous; any layout works, a head-major v -- [.., L, 32] tiles contiguous -- is the fast one).  d_head == 32,
 * L in {64,128,192,256}. */
int rf_tied_av(const void* att, const void* v, const int64_t v_strides[4], void* out, const int64_t o_strides[4], int B,
               int H, int N, int L, int d_head, void* stream);

/* Logits + softmax of the tied attention on head-major operands (rf.py:252-255), the first half of rf_tied_attention:
 *   att[b,h,i,:] = softmax_j( sum_{n,d} (w[b,h,n,i] * qscale) q[b,n,h,i,d] k[b,n,h,j,d] )      (+ att_sym as in rf_tied_softmax)
 * Same arguments as rf_tied_attention.  L in {64,128,192,256}, or L in {512,768,1024} (BASELINE.json configs[3]): long rows run
 * contraction-split over 128-query x 256-key tiles, need partial_ws (>= nsplit * B*H*L*L floats, nsplit = 1 for N <= 64,
 * doubling until N / nsplit <= 64) and take w == NULL (position weights folded into q by the projection: rf_gemm_desc.rs). */
int rf_tied_logits(const void* q, const void* k, const int64_t qk_strides[4], const float* w, const int64_t w_strides[3],
                   float qscale, void* att, float* att_sym, int64_t sym_ld, int B, int H, int N, int L, int d_head,
                   float* partial_ws, int64_t partial_ws_elems, void* stream);

/* Tied MSA-row attention core in one call (rf.py:252-265): logits + softmax, optional symmetrised map, attention . V.
 *   att[b,h,i,:] = softmax_j( sum_{n,d} (w[b,h,n,i] * qscale) q[b,n,h,i,d] k[b,n,h,j,d] ),  out = att . v
 * q / k share qk_strides {b,n,h,l}; w (fp32, may be NULL = q already scaled) has strides {b,h,n} with l contiguous: the
 * position weights of rf.py:252 are applied inside the logits kernel instead of a pass over q.  att: bf16 [B,H,L,L]
 * (caller-owned workspace and result); att_sym as in rf_tied_softmax (may be NULL).
 * partial_ws (may be NULL): fp32 workspace of partial_ws_elems elements.  With L == 256 and at least
 * 2 * B*H*L*L elements (4 * B*H*L*L when N > 128) the logits run contraction-split: workgroups of 128 query rows x 256
 * keys over ranges of <= 64 MSA rows write fp32 partial logits there and a second kernel adds them and takes the row
 * softmax (0.6x the L2 -> LDS bytes of the one-pass kernel).  Without it, or for other shapes, the one-pass kernel runs. */
int rf_tied_attention(const void* q, const void* k, const void* v, const int64_t qk_strides[4], const int64_t v_strides[4],
                      const float* w, const int64_t w_strides[3], float qscale, void* att, float* att_sym, int64_t sym_ld,
                      void* out, const int64_t o_strides[4], int B, int H, int N, int L, int d_head, float* partial_ws,
                      int64_t partial_ws_elems, void* stream);

/* The tied attention at ANY chain length (rf_version >= 12): rf_tied_softmax, rf_tied_logits, rf_tied_av and rf_tied_attention
 * with a leading dimension for the attention map.  att_ld = elements between rows of att, element (b,h,i,j) at
 * ((b*H + h)*L + i)*att_ld + j; att_ld >= L (RF_EINVAL otherwise) and att_ld % 8 == 0 (RF_EALIGN otherwise), so that every
 * row is 16-byte aligned and att_ld is a legal K for a 16-bit rf_gemm whatever L is.  The entry points above are the
 * att_ld == L case of the same code, restricted to their own lengths.
 *   - L is a run-time length: 1 <= L <= 256 for rf_tied_av_ld, rf_tied_attention_ld and the one-pass kernel of
 *     rf_tied_logits_ld (RF_EINVAL otherwise; rf_tied_logits_ld also keeps L in {512,768,1024} with att_ld == L and the
 *     workspace, as rf_tied_logits); any L >= 1 for rf_tied_softmax_ld.
 *   - rows i >= L of att are neither read nor written; columns L <= j < att_ld of every written row are written as exact
 *     zeros (consumers contract over att_ld), and rf_tied_av_ld relies on them being zeros.
 *   - no source row >= L of q, k, v or w is addressed; output rows >= L are not stored.
 *   - att_sym is [B,L,L,H] with sym_ld as in rf_tied_softmax.
 *   - w (rf_tied_logits_ld / rf_tied_attention_ld, may be NULL): strides {b,h,n} multiples of 4 as before, i.e. every row
 *     of w is 16-byte aligned: a dense [B,H,N,L] w qualifies only when L % 4 == 0, otherwise pad its rows to 4*ceil(L/4)
 *     floats (the pad values are read but reach no stored result). */
int rf_tied_softmax_ld(const float* logits, void* att, int att_dtype, int64_t att_ld, float* att_sym, int64_t sym_ld, int B,
                       int H, int L, void* stream);
int rf_tied_logits_ld(const void* q, const void* k, const int64_t qk_strides[4], const float* w, const int64_t w_strides[3],
                      float qscale, void* att, int64_t att_ld, float* att_sym, int64_t sym_ld, int B, int H, int N, int L,
                      int d_head, float* partial_ws, int64_t partial_ws_elems, void* stream);
int rf_tied_av_ld(const void* att, int64_t att_ld, const void* v, const int64_t v_strides[4], void* out,
                  const int64_t o_strides[4], int B, int H, int N, int L, int d_head, void* stream);
int rf_tied_attention_ld(const void* q, const void* k, const void* v, const int64_t qk_strides[4], const int64_t v_strides[4],
                         const float* w, const int64_t w_strides[3], float qscale, void* att, int64_t att_ld, float* att_sym,
                         int64_t sym_ld, void* out, const int64_t o_strides[4], int B, int H, int N, int L, int d_head,
                         float* partial_ws, int64_t partial_ws_elems, void* stream);

/* The contraction-split logits + softmax of the tied attention at ANY chain length 257 <= L <= 1024 (rf_version >= 20):
 *   att[b,h,i,:] = softmax_j( sum_{n,d} q[b,n,h,i,d] k[b,n,h,j,d] )      (+ att_sym as in rf_tied_softmax)
 * on 128-query x 256-key tiles, ceil(L / 128) x ceil(L / 256) of them per (b, h) and range of MSA rows.  q carries the position
 * weights (fold them in with rf_gemm_desc.rs: there is no w; qscale is accepted for symmetry with rf_tied_logits and, as there
 * with w == NULL, multiplies nothing).  q, k, qk_strides, att, att_ld, att_sym, sym_ld as in rf_tied_logits_ld: att_ld >= L
 * (RF_EINVAL) and att_ld % 8 == 0 (RF_EALIGN); rows i >= L of att are not touched, columns L <= j < att_ld of every row are exact
 * zeros, no source row >= L of q or k is addressed.  The split rule of rf_tied_logits holds: N even, split into 1, 2, 4, .. ranges
 * until a range has <= 64 rows, and a range of 4 .. 64 and an even number of rows (RF_EINVAL otherwise, as for L outside
 * 257 .. 1024 and d_head != 32).  At a length off 512 / 768 / 1024 the accepted ranges are halved further while fewer than 192
 * workgroups (B * H * tiles * ranges) would run and a half still has a multiple of 2 and at least 4 rows.  partial_ws: fp32 workspace of at least rf_tied_logits_long_ws_elems(B, H, N, L) elements,
 * 16-byte aligned (RF_EINVAL when NULL or shorter); that function returns ranges * B * H * L * 256 * ceil(L / 256), or 0 for a
 * shape the entry point refuses.  L % 256 == 0 with att_ld == L launches the whole-tile instantiations, bit for bit
 * rf_tied_logits; rf_tied_logits and rf_tied_logits_ld keep their own lengths. */
int64_t rf_tied_logits_long_ws_elems(int B, int H, int N, int L);
int rf_tied_logits_long(const void* q, const void* k, const int64_t qk_strides[4], float qscale, void* att, int64_t att_ld,
                        float* att_sym, int64_t sym_ld, int B, int H, int N, int L, int d_head, float* partial_ws,
                        int64_t partial_ws_elems, void* stream);

/* Introspection for tests and measurement tools, like rf_rowops_last_route: the kernel instantiation the calling thread's last
 * successful rf_favor_attention, rf_tied_logits_softmax, rf_tied_logits(_ld), rf_tied_logits_long, rf_tied_av(_ld), rf_tied_attention(_ld) or
 * rf_poswise_collapsed launched (-1 none; after a call that returned an error the value is unspecified).  Host-side only, no
 * kernel sees it.  rf_tied_attention(_ld) launches two kernels and leaves 1000 * (logits code) + (attention.V code).
 *   100 .. 111  rf_favor_attention, 4-wave kernel (RF_FAVOR4, and always the softmax features in the 256-row tile):
 *               100 + 4 * (tile: 0 = 64, 1 = 128, 2 = 256 rows) + 2 * (softmax features) + (tail: seq_len does not fill the tiles)
 *   112 .. 121  rf_favor_attention, 8-wave kernel: 112 + the same three terms (the softmax features end at the 128-row tile)
 *   200 .. 215  tied logits, one-pass kernel: 200 + 4 * (tile / 64 - 1) + 2 * (w != NULL) + (tail: L < tile or att_ld != L)
 *   220 / 221   tied logits, contraction-split, L = 256: w == NULL / w != NULL
 *   222 / 224 / 226   tied logits, contraction-split, L = 512 / 768 / 1024 (w == NULL); rf_tied_logits_long reports the code of
 *               its key-block count, 220 + 2 * (ceil(L / 256) - 1), at any 257 <= L <= 1024, whole tiles or tail
 *   240 .. 247  attention . V: 240 + 2 * (tile / 64 - 1) + (tail)
 *   261 .. 268  rf_poswise_collapsed: 260 + NT, NT = ceil(N / 16) row tiles (N < 16 NT: the tail instantiation of that tile count)
 *   272 / 276   rf_poswise_collapsed, 129 <= N <= 192 / 193 <= N <= 256 (NT = 12 / 16) */
int rf_attn_last_route(void);

/* Feed-forward block with its residual in ONE launch (FeedForward, rf.py:270-281, inside the residual wrappers of the
 * encoder / axial layers rf.py:284-354, 483-560):
 *   out[m,:] = residual[m,:] + W2 relu(W1 x[m,:] + b1) + b2          (fp32; out may alias residual: in place)
 *   ln_out[m,:] = gamma * (out[m,:] - mean) * rstd + beta             (optional 16-bit copy: the NEXT layer's LayerNorm)
 * The hidden activations never reach HBM.  x: 16-bit [M, D] (ldx elements between rows), D = 288 or 384, hidden % 32 == 0,
 * M % 128 == 0.  w_packed: both weight matrices in the fragment order the kernel streams (16-bit, 2 * D * hidden elements):
 * for chunk c of 32 hidden units, first D/32 * 2 pieces of W1, then D/16 pieces of W2, a piece = 64 lanes x 8 elements,
 * lane = 16 fq + fr:
 *   W1 piece (ks, ht):  element j of the lane = W1[32 c + 16 ht + fr][32 ks + 8 fq + j]          (W1: [hidden, D])
 *   W2 piece (nt):      element j of the lane = W2[row(nt, fr)][32 c + 16 (j >> 2) + 4 fq + (j & 3)]  (W2: [D, hidden]) with
 *                       row(nt, fr) = 16 nt + fr for D = 288 and, for D = 384 (an even number of column tiles per wave: the lane's
 *                       values of two tiles are 8 consecutive columns, 16-byte pieces of the LayerNorm copy),
 *                       row = 192 (nt / 12) + 32 (i >> 1) + 8 (fr >> 2) + 4 (i & 1) + (fr & 3), i = nt % 12  (ops.ffn_pack)
 * (ops.ffn_pack builds it once per module).  b1 [hidden], b2 [D], gamma / beta [D]: fp32. */
int rf_ffn_fused(const void* x, int64_t ldx, const void* w_packed, const float* b1, const float* b2, const float* residual,
                 int64_t ldr, float* out, int64_t ldo, void* ln_out, int64_t ldn, const float* ln_gamma,
                 const float* ln_beta, float ln_eps, int64_t M, int D, int hidden, void* stream);

/* PositionWiseWeightFactor in collapsed form on the matrix pipe (rf.py:205-217):
 *   w[b,h,n,l] = softmax_n( scale * sum_c xn[b,n,l,c] * u[b,l,h,c] ),   u[b,l,h,:] = W_k[h*dh:(h+1)*dh, :]^T to_q(x_0)[b,l,h,:]
 * (to_k's bias is constant in n and cancels in the softmax, so the to_k projection over all N rows is never formed).
 * xn: bf16 [B,N,L,D]; u: bf16 [B,L,H,D]; w: fp32 [B,H,N,L].  H <= 16, D % 32 == 0, 1 <= N <= 256 (rf_version >= 20: before,
 * N / 16 in {1..8, 12, 16} was required).  The kernel walks the MSA rows in MFMA tiles of 16, NT = the smallest of 1..8, 12, 16
 * that holds ceil(N / 16); a depth that does not fill them runs the tail instantiation: no row >= N of xn is addressed, none of w
 * is written, and N == 16 NT launches what it always did. */
int rf_poswise_collapsed(const void* xn, const void* u, float* w, int B, int N, int L, int D, int H, float scale,
                         void* stream);

/* Fused OuterProductMean (rf.py:412-427): out[b,i,j,:] = Linear(LayerNorm_1024(sum_n x[b,n,i,:] (x) y[b,n,j,:])) in one
 * kernel; the 1024-wide feature tensor never exists in HBM.  xt / yt: bf16 [B, L, 32, N] (MSA depth contiguous);
 * wprime: 16-bit [16, Dout, 64] = W * gamma (LayerNorm affine folded in) stored CHUNK-MAJOR: wprime[c][o][8 uu + vv] =
 * (W gamma)[o][k], k = (8 (c / 4) + uu) * 32 + 8 (c % 4) + vv -- the 64 features one chunk of the kernel contracts over are one
 * 128-byte line per output column; s[o] = sum_k wprime[o,k] (fp32, of the 16-bit values);
 * c[o] = sum_k W[o,k] beta[k] + bias[o]; out: fp32 [B, L, L, Dout]:
 *     out = rstd * (sum_k co_k wprime[o,k] - mean * s[o]) + c[o],   mean / rstd over the 1024 features in fp32.
 * Supported: P == 32, Dout == 288, N in {64, 128}, any L >= 1 (RF_EINVAL otherwise: rf_gemm with RF_ACT_BLOCK_LN32 + rf_gemm;
 * rf_version >= 19: before, L % 16 == 0 was required).  This is rf_outer_product_ln_linear_rect with Li = Lj = L; a picture of
 * whole tiles (L % 16 == 0) runs the instruction stream it always ran.
 * Optional tail (PairUpdateWithMsa.ln_coevol_feat, rf.py:443,486): with y != NULL the kernel applies a second LayerNorm
 * (ln2_gamma / ln2_beta [Dout], ln2_eps) over the Dout outputs of every pair and writes 16-bit y[(b,i,j) * y_ld + o] INSTEAD of
 * `out` (which may then be NULL): the fp32 result and the separate LayerNorm pass over it disappear as well.  y: 16-byte
 * aligned, y_ld % 8 == 0 (rows leave as 16-byte pieces). */
int rf_outer_product_ln_linear(const void* xt, const void* yt, const void* wprime, const float* s, const float* c, float* out,
                               int B, int L, int N, int P, int Dout, float eps, const float* ln2_gamma, const float* ln2_beta,
                               float ln2_eps, void* y, int64_t y_ld, void* stream);

/* The same kernel on a RECTANGULAR picture of any size (rf_version >= 19): rows i of xt against columns j of yt.
 *   xt: 16-bit [B, Li, 32, N];  yt: 16-bit [B, Lj, 32, N];  out: fp32 [B, Li, Lj, Dout];  y: 16-bit, y[((b Li + i) Lj + j) y_ld + o];
 *   wprime / s / c / eps / ln2_* / y_ld as in rf_outer_product_ln_linear.
 * A block of pair rows (the row-sharded forward: Li = the rank's rows, Lj = L) is one call; so is a chain whose length is no
 * multiple of the tile.  The kernel walks ceil(Li / 16) x ceil(Lj / 8) tiles of 16 x 8 pairs per sample.  In a tile that hangs
 * over the picture the residues beyond it are neither read nor written: their operand rows are fetched from the LAST VALID
 * residue of the same sample instead (no address leaves [b, 0 .. Li - 1] of xt or [b, 0 .. Lj - 1] of yt), the arithmetic of such
 * a pair runs on that duplicate and stays finite, and every store -- fp32 rows of `out`, 16-byte pieces of the rows of `y` -- is
 * predicated on (i, j) lying inside the picture.  Every element out[b, i, j, 0 .. Dout - 1] (or y[..., 0 .. Dout - 1]) with
 * b < B, i < Li, j < Lj is written and nothing else is: columns Dout .. y_ld - 1 of `y` and memory before / behind the addressed
 * block keep their contents.  A pair's result depends on its own operand rows only (bit-identical whichever picture holds it).
 * The MSA depth stays N in {64, 128}: a shallower MSA is zero-padded by the caller (zeros add nothing to the sum over n); a
 * deeper one would need 192 KB of operand buffers in the 160 KB of LDS and stays on the rf_gemm route.
 * RF_EINVAL: a NULL operand, B / Li / Lj <= 0, P != 32, Dout != 288, N not in {64, 128}, neither `out` nor `y`, more than 2^31 - 1
 * tiles, or with y != NULL: ln2_gamma / ln2_beta NULL, y_ld < Dout, y_ld % 8 != 0, y / ln2_gamma / ln2_beta not 16-byte aligned.
 * RF_EALIGN: xt, yt, wprime, s, c or out not 16-byte aligned. */
int rf_outer_product_ln_linear_rect(const void* xt, const void* yt, const void* wprime, const float* s, const float* c, float* out,
                                    int B, int Li, int Lj, int N, int P, int Dout, float eps, const float* ln2_gamma,
                                    const float* ln2_beta, float ln2_eps, void* y, int64_t y_ld, void* stream);

/* PositionWiseWeightFactor core (rf.py:205-217): w[b,n,h,l] = softmax_n( scale * sum_{c<dlen} q0[b,l,h,c]*k[b,n,l,h,c] ).
 * q0: [B,L,H*dlen] (dtype q0_dtype, ld q0_ld); k: T rows [B,N,L,*] of ld k_ld, head h at column k_col0 + h*k_hstride.
 *   - direct form:    q0 = to_q(row 0), k = to_k(x), dlen = k_hstride = d_head;
 *   - collapsed form: q0 = to_q(row 0) W_k (one [B*L,d]x[d,d] GEMM), k = x itself, dlen = d, k_hstride = 0
 *     (the to_k GEMM over all N rows disappears; its bias is constant in n and drops out of the softmax).
 * w (fp32 [B,N,H,L]) may be NULL.  When q_scale != NULL the kernel also does the fused `q = q * w * qscale` of
 * rf.py:252 in place on q_scale: T [B,N,L,*] (ld qs_ld, head h = columns qs_col0 + h*qs_dh .. +qs_dh). */
int rf_poswise(const void* q0, int q0_dtype, int64_t q0_ld, const void* k, int64_t k_ld, int k_col0, int k_hstride,
               int dlen, float* w, void* q_scale, int64_t qs_ld, int qs_col0, int qs_dh, int dtype, int B, int N, int L,
               int H, float scale, float qscale, void* stream);

/* y[b,l,:] = sum_n w[b,n,0,l] * x[b,n,l,:]   (rf.py:723, rf.py:797); x T [B,N,L,D], y fp32 [B,L,D] (ld y_ld) */
int rf_weighted_msa_sum(const void* x, int dtype, const float* w, float* y, int64_t y_ld, int B, int N, int L, int D,
                        void* stream);

/* InstanceNorm2d(affine, eps) on NHWC (rf.py:453,457; resnet.py:29,39,63) in two steps:
 * stats: sums[b,c,0..1] = (sum, sumsq) over the L*L pixels (fully written: no zeroing needed);
 * apply: y = act( (x-mean)*rstd*gamma + beta [+ residual] ) ; act = RF_ACT_NONE | RF_ACT_ELU. */
/* workspace (MANDATORY, rf_instnorm_ws_bytes bytes): per-block partial sums reduced in a fixed order -- the library has no
 * atomic accumulation anywhere, results are bitwise reproducible run to run; NULL / too small -> RF_EINVAL. */
int64_t rf_instnorm_ws_bytes(int B, int64_t HW, int C);
int rf_instnorm_stats(const void* x, int x_dtype, void* sums /* 2*B*C doubles */, int B, int64_t HW, int C, void* workspace,
                      int64_t ws_bytes, void* stream);
/* gamma == beta == NULL: centre only, y = x - mean over the picture (no scaling; PredictionHead operand conditioning). */
int rf_instnorm_apply(const void* x, int x_dtype, const void* sums, const float* gamma, const float* beta, float eps,
                      const float* residual, int act, void* y, int y_dtype, void* y2, int y2_dtype, int B, int64_t HW,
                      int C, void* stream);

/* ---- operand conditioning of the 16-bit modes (csrc/condition.hip): exact algebra, the function computed is unchanged ----
 * At random init every stream is a large per-sample constant vector plus a position-dependent part 10-30x smaller, and the
 * InstanceNorms (rf.py:453,457; resnet.py:29,39,63) keep only the latter; an operand rounded to 16 bits WITH the constant is
 * 10-30x coarser than the information that survives.  PairUpdateWithMsa (rf.py:476-498), PredictionHead (rf.py:1130-1172)
 * and the structure track's embeddings remove the constant before the rounding and add W * constant back in fp32:
 *   W (x - m) + (b + W m) == W x + b;   conv3x3(x - m) + [taps outside the picture] == conv3x3(x) - const (InstanceNorm drops it).
 * mean[b,c] = sums[b,c,0] / HW from the sums of rf_instnorm_stats (fp32 [B,C]). */
int rf_instnorm_mean(const void* sums, float* mean, int B, int64_t HW, int C, void* stream);
/* the same mean straight from fp32 NHWC x (C % 4 == 0, 16-byte aligned): vectorised, no atomics; workspace of
 * rf_channel_mean_ws_bytes bytes (MANDATORY: per-block partial sums, added in a fixed order). */
int64_t rf_channel_mean_ws_bytes(int B, int64_t HW, int C);
int rf_channel_mean(const float* x, float* mean, int B, int64_t HW, int C, void* workspace, int64_t ws_bytes, void* stream);
/* an ESTIMATE of that mean from nsample evenly spaced rows of x [B,R,C] (fp32 or 16-bit): the identities hold for any constant,
 * the attention layers condition their value operand with it (model.py: _value_conditioning). */
int rf_sample_mean(const void* x, int x_dtype, float* mean, int B, int64_t R, int C, int nsample, void* stream);
/* y[b,p,c] = x[b,p,c] - mean[b,c]; x fp32 [B,HW,C], y fp32 or the 16-bit type (may alias x when fp32); C % 4 == 0, 16-byte
 * aligned pointers. */
int rf_center_apply(const float* x, const float* mean, void* y, int y_dtype, int B, int64_t HW, int C, void* stream);
/* small tensors: mean[b,c] = mean over the R rows of x[b] (fp32 [B,R,C]) and x -= mean, in place (one block per sample). */
int rf_center_rows(float* x, float* mean, int B, int R, int C, void* stream);
/* the constant's way through a weight matrix (w fp32 [N, ldw]; mean fp32 [B,K]; bias fp32 [N] or NULL):
 *   sum_seg != 0: out[b,n]   = bias[n] + sum_{s<nseg} sum_{k<K} w[n, k0 + s*seg_stride + k] * mean[b,k]
 *   sum_seg == 0: out[b,s,n] = bias[n] +                sum_{k<K} w[n, k0 + s*seg_stride + k] * mean[b,k]   (e.g. the 9 taps
 *   of a 3x3 convolution stored [Co, 9*Ci]: nseg 9, seg_stride Ci). */
int rf_fold_mean(const float* w, int64_t ldw, int k0, int K, int nseg, int64_t seg_stride, int sum_seg, const float* mean,
                 const float* bias, float* out, int B, int N, void* stream);
/* 3x3 'same' (zero-padded) convolution of a centred picture: y[b,i,j,:] -= sum of taps[b, kh*3+kw, :] over the taps whose
 * source pixel (i+(kh-1)d, j+(kw-1)d) lies outside the picture, so that y == conv3x3(x) - (sum of all taps) everywhere.
 * y NHWC fp32 or 16-bit, in place; taps fp32 [B,9,C] (rf_fold_mean); edges: which sides of this block are sides of the picture
 * (1 top | 2 bottom | 4 left | 8 right; 15 for a whole picture, a row block of a sharded picture has neighbours). */
int rf_conv3x3_border_fix(void* y, int y_dtype, const float* taps, int B, int H, int W, int C, int dilation, int edges,
                          void* stream);

/* MsaEmbedding (rf.py:106-120): y[b,n,l,:] = emb[msa[b,n,l]] + pe[aa_idx[b,l]] + qenc[n==0 ? 0 : 1]; fp32 out. */
int rf_msa_embed(const int64_t* msa, const int64_t* aa_idx, const float* emb, const float* pe, const float* qenc,
                 float* y, int B, int N, int L, int D, void* stream);

/* PairEmbedding (rf.py:123-181, 79-103) with the 289->d Linear factorised into two 21-row tables:
 * y[b,i,j,:] = tl[seq[b,j]] + tr[seq[b,i]] + wsep*log(|idx_i-idx_j|+1) + bias + [pe[idx_i] | pe[idx_j]]. */
int rf_pair_embed(const int64_t* seq, const int64_t* aa_idx, const float* tl, const float* tr, const float* wsep,
                  const float* bias, const float* pe, float* y, int B, int L, int D, void* stream);

/* Generic strided copy / cast / transpose (einops rearrange of the reference, e.g. rf.py:258,403,408,593):
 * y[i0,i1,i2,i3] = x[...] over a 4-D index space with element strides per side. */
int rf_copy4d(const void* x, int x_dtype, const int64_t xs[4], void* y, int y_dtype, const int64_t ys[4],
              const int64_t dims[4], void* stream);

/* y = a*x + b*z  elementwise fp32/T (n elements; z may be NULL) */
int rf_axpby(const void* x, int x_dtype, float a, const void* z, int z_dtype, float b, void* y, int y_dtype,
             int64_t n, void* stream);

/* y[r,:] = x[r,:] * w[r]  (msa_proj * position weight, rf.py:472); x, y T [rows, D]; y may alias x */
int rf_scale_rows(const void* x, void* y, int dtype, const float* w, int64_t rows, int D, void* stream);

/* y[0..n) = value (T); y 16-byte aligned.  Zero / one initialisation of caller-owned buffers without a framework kernel. */
int rf_fill(void* y, int dtype, float value, int64_t n, void* stream);

/* Input validation of RoseTTAFold.forward (the reference raises IndexError from nn.Embedding / tensor indexing,
 * rf.py:73,98,115-119,155): flags[0] = a token outside [0, d_input), flags[1] = an aa_idx outside [0, max_len),
 * flags[2] = aa_idx not strictly increasing inside a sample (the kNN edge-capacity bound then does not hold, rf.py:841-852).
 * msa / seq / aa_idx may each be NULL (skipped).  flags: 3 x int32, zeroed by the caller. */
int rf_check_inputs(const int64_t* msa, int64_t n_msa, const int64_t* seq, int64_t n_seq, const int64_t* aa_idx,
                    int64_t n_idx, int L, int d_input, int max_len, int32_t* flags, void* stream);

/* y[r, col0 + c] = (idx[r] == c), c < n_classes  (F.one_hot(seq, 21), rf.py:1276); y T with leading dim y_ld */
int rf_onehot(const int64_t* idx, void* y, int dtype, int64_t y_ld, int col0, int n_classes, int64_t rows, void* stream);

/* y[(b,i,j)*y_ld + col] = clamp(sign(d)*log(|d|+1), 0, 5.5), d = aa_idx[b,i]-aa_idx[b,j]  (rf.py:746-749) */
int rf_seqsep_feature(const int64_t* aa_idx, void* y, int dtype, int64_t y_ld, int col, int B, int L, void* stream);

/* Stand-alone positional encodings, fp32: two_d == 0: SinusoidalPositionalEncoding.forward (rf.py:72-76)
 * y[b,n,l,:] = x + pe[aa_idx[b,l]] (pe [max_len, D]); two_d != 0: SinusoidalPositionalEncoding2D.forward (rf.py:95-103)
 * y[b,i,j,:] = x + [pe[aa_idx[b,i]] | pe[aa_idx[b,j]]] (N == L, pe [max_len, D/2]).  aa_idx must be in range. */
int rf_add_pos_enc(const float* x, const int64_t* aa_idx, const float* pe, float* y, int B, int N, int L, int D, int two_d,
                   void* stream);

/* FAVOR+ softmax-kernel features (performer-pytorch softmax_kernel as called at rf.py:313-318; third party,
 * parity unpinned).  One workgroup per (sequence, head) S.  dash = (d^-1/4 x) P^T from rf_gemm, T, laid out
 * [S][n][m_pad] (transposed=0) or [S][m_pad][n] (transposed=1).  Row r of S in x (T) starts at
 * s0*xs[0]+s1*xs[1]+s2*xs[2]+r*xs[3] with S = (s0*n1+s1)*n2+s2.
 * y = m^-1/2 * (exp(dash - |x|^2 d^-1/2 /2 - max) + eps) for features < m, 0 for the padded ones.
 * is_query: max over the feature axis per row; else over (n, m) per S.  y may alias dash. */
int rf_favor_softmax_features(const void* dash, const void* x, const int64_t xs[4], int n1, int n2, void* y, int dtype,
                              int64_t S, int n, int m, int m_pad, int dh, int is_query, int transposed, float eps,
                              void* stream);

/* Fused FAVOR+ attention (performer-pytorch SelfAttention.fast_attention as called at rf.py:313-318 [softmax
 * kernel] and rf.py:505-518 [generalized ReLU kernel]; third party, parity unpinned): for every (batch b, outer index
 * o, head h) item the sequence s in [0,seq_len) is attended with
 *     q' = phi(q Pc^T), k' = phi(k Pc^T), out = (q' (k'^T v)) / (q' . sum_s k')
 * entirely on-chip.  qkv: bf16 rows holding q|k|v at column offsets q_off/k_off/v_off (+ h*dim_head); the row of
 * (b,o,s) of head h starts at b*x_strides[0] + o*x_strides[1] + s*x_strides[2] + h*x_strides[3] (elements); out
 * (bf16) likewise with o_strides, head h at column h*dim_head.  pc: bf16 [288][64] projection matrix pre-scaled by dim_head^-1/4, rows >= 266 zero.
 * Supported: dim_head 64, n_features 266; any seq_len >= 1 with the ReLU kernel (up to 256 rows in one 64- / 128- / 256-row
 * tile, longer sequences walked in 256-row chunks with a partial last one), 1 <= seq_len <= 256 with the softmax kernel (its
 * key maximum spans the whole sequence; longer: RF_EINVAL, use the unfused chain of rf_gemm + rf_favor_softmax_features +
 * rf_linattn_normalize).  Rows s >= seq_len of an item are neither read nor written: they may belong to another sequence
 * or lie outside the buffers.  softmax_kernel != 0: exp features with the library's
 * stabilisers (per-row max for q, per-(b,o,h) max for k) and eps; else relu(x)+eps.
 * With softmax_kernel != 0 the kernel exponentiates with exp2, so pc must be dim_head^-1/4 * log2(e) * P (with
 * softmax_kernel == 0: dim_head^-1/4 * P), and the features are
 *     phi(x) = exp2(x Pc^T - |x|^2 dim_head^-1/2 log2(e) / 2 - max) + eps,
 * the maximum of x Pc^T over the 266 features per row for q, over all rows s < seq_len and the 266 features per item for k. */
int rf_favor_attention(const void* qkv, const void* pc, void* out, const int64_t x_strides[4],
                       const int64_t o_strides[3], int q_off, int k_off, int v_off, int n_b, int n_o, int n_h,
                       int seq_len, int dim_head, int n_features, int softmax_kernel, float eps, void* stream);

/* Linear-attention normalisation (performer-pytorch linear_attention): y[r, :dh] = num[r, :dh] / num[r, dh]
 * where column dh of `num` carries q'.ksum (the context matrix has a ones-row appended). */
int rf_linattn_normalize(const float* num, int64_t num_ld, void* y, int y_dtype, int64_t y_ld, int64_t rows, int dh,
                         void* stream);

/* Outer-product features (rf.py:476-485): feat[b,i,j, c0 + (0..2p)] = msa1d[b,i,:], feat[.., c0+2p + (0..2p)] = msa1d[b,j,:] */
int rf_tile_1d_feats(const float* msa1d, void* feat, int dtype, int64_t feat_ld, int c0, int B, int L, int P2,
                     void* stream);

/* GraphTransformer attention core (rf.py:647-662) for one layer: q,k,v T [B,L,H*d]; e T [B,L,L,H*d];
 * out fp32 [B,L,H*d] = sum_j softmax_j(scale*(q.k_j + q.e_ij)) * (v_j + e_ij). */
int rf_graph_attention(const void* q, const void* k, const void* v, const void* e, int dtype, float* out, int B, int L,
                       int H, int d, float scale, void* stream);

/* Training-mode form of rf_graph_attention: dropout(p) on the attention probabilities (att_dropout, rf.py:628,658); mask =
 * Philox4x32-10(seed, offset + element / 4) over the [B, H, L, L] map, like rf_dropout. */
int rf_graph_attention_dropout(const void* q, const void* k, const void* v, const void* e, int dtype, float* out, int B, int L,
                               int H, int d, float scale, float p, uint64_t seed, uint64_t offset, void* stream);

/* rf_graph_attention under an edge mask (the reference's edge_mask, rf.py:632-655): mask uint8 [B,L,L], nonzero = the edge
 * (i, j) exists.  A row with at least one edge takes its softmax over its edges only: a masked column gets probability exactly 0
 * and k, v, e at it are not read (the reference adds -1e9 to its logit, which underflows exp to 0: the same as -inf).  A row
 * with no edge gets the uniform 1/L over all L columns (every logit 0).  That is what the reference computes whenever every
 * scaled logit of the row lies in (-32, 32): the float32 spacing at 1e9 is 64, so x - 1e9 rounds to -1e9 for all of them; outside
 * that bound the reference's empty row is quantisation noise of the -1e9 trick and is not followed.  The work of a row is
 * proportional to its degree; columns are taken in ascending order, so an all-ones mask gives rf_graph_attention's bits.
 * p = 0: no dropout; 0 < p < 1: rf_graph_attention_dropout's mask (the same keep/drop decision per [b, h, i, j] element).
 * RF_EINVAL: mask NULL, p outside [0, 1), H*d > 256, d > 64 or not a power of two, (H*L + L + 8) * 4 bytes of LDS > 64 KB. */
int rf_graph_attention_masked(const void* q, const void* k, const void* v, const void* e, int dtype, const uint8_t* mask,
                              float* out, int B, int L, int H, int d, float scale, float p, uint64_t seed, uint64_t offset,
                              void* stream);

/* nn.Dropout for the training-mode forward (rf.py:18-28, 76, 217, 265-281, 346, 455, 567, 592, 1138; resnet.py:30):
 * y[e] = keep[e] ? x[e] / (1 - p) : 0 over n elements of dtype (fp32 or the build's 16-bit type; y may alias x), keep[e] =
 * word (e % 4) of Philox4x32-10(key = seed, counter = offset + e / 4) >= p * 2^32.  Stateless: the caller gives every call of a
 * forward its own offset range (ceil(n / 4) counters), so a seed reproduces the forward bit for bit.  0 <= p < 1. */
int rf_dropout(const void* x, void* y, int dtype, float p, uint64_t seed, uint64_t offset, int64_t n, void* stream);

/* MsaUpdateWithPairAndCoord attention map (rf.py:899-914): att T [B,4,L,L] = softmax_j(q.k*1 + (dist<bin ? 0 : -1e9));
 * q (pre-scaled by the caller) and k: fp32 [B,L,H*dq]; ca: fp32 xyz [B,L,3,3] (CA = atom 1). */
int rf_dist_masked_attention(const float* q, const float* k, const float* xyz, const float* bins, void* att,
                             int att_dtype, int B, int L, int H, int dq, void* stream);

/* ---- SE(3) structure module (rf.py:752-862, se3_modules.py:83-171, ea/modules.py) -------------------------- */

/* kNN graph (rf.py:823-862) in dense form: mask[b,i,j] = 1 iff edge i->j exists
 * (j among the k nearest CA of i, ties broken by lower j, or |idx_i-idx_j| < kmin; self loops only when k >= L). */
int rf_knn_mask(const float* xyz, const int64_t* aa_idx, uint8_t* mask, int B, int L, int k, int kmin, void* stream);

/* Compact the dense mask into an edge list sorted by (b,i,j) (row-major torch.where order, rf.py:853):
 * src/dst node ids (b*L+i / b*L+j), eid[b,i,j] = edge id or -1.  count: 2 x int32 -- count[0] = min(edges, capacity)
 * (what consumers iterate over), count[1] = the true number of edges.  src/dst hold `capacity` entries; an edge whose
 * id would be >= capacity is DROPPED (eid = -1, nothing written) and shows up as count[1] > capacity, so the caller's
 * buffers are never overrun.  For strictly increasing aa_idx and finite coordinates a row has at most
 * min(L, k + 2*(kmin-1)) edges; otherwise use capacity B*L*L.  row_ws: 2*B*L int32 scratch. */
int rf_edges_from_mask(const uint8_t* mask, int32_t* src, int32_t* dst, int32_t* eid, int32_t* count, int32_t* row_ws,
                       int B, int L, int64_t capacity, void* stream);

/* Per-edge geometry (ea/modules.py:26-108): d = CA[dst]-CA[src]; r; real SH Y0..Y2 and the four equivariant
 * bases folded with the Q_J constants: basis layout [E, 1+3+3+27] floats = (0,0)[1] (0,1)[3x1] (1,0)[1x3] (1,1)[3x3x3];
 * also feat[e, :] = [w(edge embedding, d_edge) | r] with leading dim feat_ld. */
int rf_se3_edge_geometry(const float* xyz, const float* edge_emb, const int32_t* src, const int32_t* dst,
                         const int32_t* count, float* basis, float* feat, int64_t feat_ld, int L, int d_edge,
                         int64_t capacity, void* stream);

/* Partial convolution message (ea/modules.py:612-641 + 287-325): for output degree `dout` with `mo` channels,
 * msg[e, o, a] = sum_{di} sum_{i,b,f} R_{di}[e, o, i, f] * basis_{di,dout}[e, a, b, f] * h_{di}[src[e], i, b].
 * R0/R1: radial outputs (fp32, [E, mo*mi0*nf0] and [E, mo*mi1*nf1]); h0 [V, mi0], h1 [V, mi1, 3]. */
int rf_se3_message(const float* R0, const float* R1, const float* basis, const float* h0, const float* h1,
                   const int32_t* src, const int32_t* count, float* msg, int mo, int dout, int mi0, int mi1,
                   int64_t capacity, void* stream);

/* Fused form (round 4): the whole radial MLP (RadialFunc, ea/modules.py:246-284: Linear(d_edge+1 -> 32) -> LayerNorm
 * -> ReLU -> Linear(32 -> 32) -> LayerNorm -> ReLU -> Linear(32 -> mo*mi*nf)) evaluated per edge inside the message kernel from
 * feat [E, feat_ld] (= [edge embedding | r], ki = d_edge + 1 columns): neither the hidden vectors nor the radial outputs R
 * are written.  net_di: the packed fp32 parameters of net (di, dout), 16-byte aligned,
 *   [W1^T: ki x 32][b1 32][ln1 gamma 32][ln1 beta 32][W2^T: 32 x 32][b2 32][ln2 gamma 32][ln2 beta 32][W3: rows x 32][b3: rows],
 * rows = mo*mi_di*nf_di ordered (o, i, f) as the reference's view(-1, mo, 1, mi, 1, nf) (ea/modules.py:283); mi_di = 0 / NULL:
 * input degree absent.  rf_se3_radial_message_supported tells whether a shape has an instance (else: rf_gemm + rf_se3_message). */
int rf_se3_radial_message_supported(int mo, int dout, int mi0, int mi1, int ki);
int rf_se3_radial_message(const float* feat, int64_t feat_ld, int ki, const float* net0, const float* net1, const float* basis,
                          const float* h0, const float* h1, const int32_t* src, const int32_t* count, float* msg, int mo,
                          int dout, int mi0, int mi1, float ln_eps, int64_t capacity, void* stream);

/* Graph attention (ea/modules.py:738-774): e = <k_edge, q[dst]>/sqrt(nfeat) per head, softmax over incoming edges
 * of each dst node, out[dst] = sum a * v.  k/v per-edge: k0 [E,mk0] k1 [E,mk1,3] v0 [E,mv0] v1 [E,mv1,3]; q per node.
 * One wave per (dst node, head) walks column dst of the dense eid map in fixed order (deterministic).
 * out0 / out1 rows are out0_ld / out1_ld floats apart (0 = packed: mv0 / 3*mv1), so the result can land in the leading
 * channels of the skip-concatenation buffer (GCat, ea/modules.py:903-928). */
int rf_se3_attention(const float* k0, const float* k1, const float* q0, const float* q1, const float* v0,
                     const float* v1, const int32_t* eid, float* out0, float* out1, int heads, int mk0, int mk1,
                     int mv0, int mv1, int V, int L, int64_t out0_ld, int64_t out1_ld, void* stream);

/* GNormBias (ea/modules.py:391-406): y = relu(|v| + b) * v/|v| per channel, v [V, m, 2d+1]. */
int rf_se3_norm_bias(const float* v, const float* bias, float* y, int64_t V, int m, int deg, void* stream);

/* GAttentiveSelfInt front (ea/modules.py:446-455): s[v, a*m+b] = sign-preserving clamp(<v_a, v_b>, 1e-12). */
int rf_se3_gram(const float* v, float* s, int64_t V, int m, int deg, void* stream);
/* GAttentiveSelfInt back (ea/modules.py:458-471): y[v,o,:] = sum_m softmax_m(att[v,o,m]) * x[v,m,:]. */
int rf_se3_attn_apply(const float* att, const float* x, float* y, int64_t V, int m_out, int m_in, int deg,
                      void* stream);

/* type-1 SE(3) input (rf.py:807): y[r,a,:] = xyz[r,a,:] - xyz[r,CA,:] */
int rf_center_ca(const float* xyz, float* y, int64_t nres, void* stream);

/* Coordinate update (rf.py:816-819): xyz_out from xyz and displacement [B*L,3,3]. */
int rf_coord_apply(const float* xyz, const float* disp, float* xyz_out, int64_t nres, void* stream);

/* ---- backward pass of PredictionHead and its ResNets (csrc/backward.hip; resnet.py, rf.py:1130-1172) ----------------------
 * Input gradients of the convolutions and Linears run on rf_gemm (a stride-1 "same" 3x3 convolution's input gradient is the
 * same convolution with the kernel rotated 180 degrees and its in / out channels swapped); these are the other pieces.
 * Every reduction goes through per-block partials in the caller's workspace, added in a fixed order: no atomics, bitwise
 * reproducible run to run.  The float32 matmul precision ("high", RF_F32X3) does not apply here: RF_F32 is exact fp32.
 *
 * Weight gradient of a stride-1 "same" convolution on NHWC tensors, fp32 result:
 *   dw[co][tap][ci] = alpha * sum_{b,p} dy[b,p,co] * x[b, p + delta(tap), ci]     (zero outside the picture)
 *   dbias[co]       = alpha * sum_{b,p} dy[b,p,co]                                 (dbias may be NULL)
 * dy [B,H,W,Co], x [B,H,W,Ci], both of `dtype`: the library's 16-bit type (MFMA, fp32 accumulation; Co % 8 == 0, Ci % 8 == 0,
 * 16-byte aligned, else RF_EALIGN) or RF_F32 (exact fp32).  taps = 9: 3x3 kernel, dilation 1..8, tap = 3*(di+1)+(dj+1) (the
 * k order of RF_AMODE_CONV3X3, so dw is the forward's [Co][9*Ci] weight layout); taps = 1: 1x1 convolution / Linear over
 * B*H*W rows (dilation ignored).  Workspace (MANDATORY): rf_conv_wgrad_ws_bytes bytes (0 = unsupported arguments). */
int64_t rf_conv_wgrad_ws_bytes(int dtype, int B, int H, int W, int Co, int Ci, int taps);
int rf_conv_wgrad(const void* dy, const void* x, int dtype, float* dw, float* dbias, int B, int H, int W, int Co, int Ci, int taps,
                  int dilation, float alpha, void* workspace, int64_t ws_bytes, void* stream);
/* InstanceNorm2d(affine) backward on NHWC [B, HW, C] (statistics pass + apply pass), for y = gamma * xhat + beta with xhat from
 * x (the saved input the forward normalised, fp32 or 16-bit) and `sums` (the forward's rf_instnorm_stats, eps as there):
 *   ge = g * (act_out ? (act_out > 0 ? 1 : act_out + 1) : 1)        g fp32: gradient of the output; act_out: the saved output
 *                                                                  of an ELU that followed the norm (NULL: none)
 *   dx = gamma / sigma * (ge - mean ge - xhat * mean(ge xhat))      (dx of dx_dtype: fp32 or the 16-bit type)
 *   dgamma[c] = sum_{b,p} ge xhat, dbeta[c] = sum_{b,p} ge           (either may be NULL)
 *   ge_out = ge (fp32, may alias g; NULL: not written): the gradient of a residual added before the ELU
 * Workspace (MANDATORY, 16-byte aligned): rf_instnorm_ws_bytes(B, HW, C) rounded up to 16, plus 16 * B * C bytes. */
int rf_instnorm_bwd(const float* g, const void* act_out, int act_dtype, const void* x, int x_dtype, const void* sums,
                    const float* gamma, float eps, void* dx, int dx_dtype, float* ge_out, float* dgamma, float* dbeta, int B,
                    int64_t HW, int C, void* workspace, int64_t ws_bytes, void* stream);
/* LayerNorm backward over rows of D <= 1024 (fp32 x, the forward's input; g fp32 gradient of the output; statistics recomputed
 * in fp32 like rf_layernorm):  dx = rstd * (g gamma - mean(g gamma) - xhat * mean(g gamma xhat))  (dx_dtype fp32 / 16-bit);
 * dgamma[c] = sum_rows g xhat, dbeta[c] = sum_rows g (either may be NULL).  Workspace: rf_layernorm_bwd_ws_bytes bytes. */
int64_t rf_layernorm_bwd_ws_bytes(int64_t rows, int D);
int rf_layernorm_bwd(const float* x, const float* g, const float* gamma, float eps, void* dx, int dx_dtype, float* dgamma,
                     float* dbeta, int64_t rows, int D, void* workspace, int64_t ws_bytes, void* stream);
/* LayerNorm forward and backward of operand-typed rows in one pass (OuterProductMean's backward: x = the recomputed outer
 * products, g = the gradient behind the Linear, both of `dtype` = the 16-bit type or RF_F32, as the GEMMs wrote them):
 *   z  = xhat gamma + beta                                         (of dtype: the weight gradient's operand)
 *   dx = rstd * (g gamma - mean(g gamma) - xhat * mean(g gamma xhat))   (of dtype: the following contractions' operand)
 *   dgamma[c] (+)= sum_rows g xhat,  dbeta[c] (+)= sum_rows g       (fp32, either may be NULL; accumulate != 0: added to
 *                                                                   what they hold, so a caller can walk a tensor in pieces)
 * Statistics are recomputed in fp32 from x (two-pass, like rf_layernorm); nothing of the forward is needed.  dx may alias g and
 * z may alias x.  D <= 1024, D % 8 == 0 (16-bit) / D % 4 == 0 (fp32), 16-byte aligned tensors, else RF_EALIGN.  The column sums
 * go through per-block partials added in block order (no atomics).  Workspace: rf_layernorm_bwd_fused_ws_bytes bytes. */
int64_t rf_layernorm_bwd_fused_ws_bytes(int64_t rows, int D);
int rf_layernorm_bwd_fused(const void* x, const void* g, int dtype, const float* gamma, const float* beta, float eps, void* dx,
                           void* z, float* dgamma, float* dbeta, int accumulate, int64_t rows, int D, void* workspace,
                           int64_t ws_bytes, void* stream);
/* out[0] = max_e |x[e]| over n fp32 elements (the power-of-two gradient scale of the fp16 build); workspace >= 4096 bytes. */
int rf_absmax(const float* x, int64_t n, float* out, void* workspace, int64_t ws_bytes, void* stream);

/* ---- backward pass of the pair axial attention (csrc/backward.hip; model.py PerformerSelfAttention / FeedForward,
 * rf.py:501-528) -------------------------------------------------------------------------------------------------------------
 * The products of the FAVOR+ and feed-forward backward run on rf_gemm and rf_conv_wgrad; these are the elementwise pieces.
 *
 * Linear-attention normalisation backward, for out = num[r, :dh] / num[r, dh] (rf_linattn_normalize), g fp32 = d out:
 *   dnum[r, c] = g[r, c] / num[r, dh]  (c < dh),  dnum[r, dh] = -sum_c g[r, c] out[r, c] / num[r, dh],  dnum[r, dh+1 .. dnum_ld) = 0
 * num fp32 (row stride num_ld > dh), g fp32 (row stride g_ld >= dh), dnum of dtype (row stride dnum_ld > dh); dh <= 64. */
int rf_linattn_normalize_bwd(const float* num, int64_t num_ld, const float* g, int64_t g_ld, void* dnum, int dtype,
                             int64_t dnum_ld, int64_t rows, int dh, void* stream);
/* ReLU feature-map backward of the generalized FAVOR+ kernel (phi = relu(z) + eps for columns < nvalid, 0 beyond):
 *   dz[r, c] = (c < nvalid && z[r, c] > 0) ? dphi[r, c] : 0      dphi, z fp32 [rows, ld]; dz of dtype [rows, ld]
 * z is the fp32 pre-activation (the mask is never taken from a rounded phi). */
int rf_relu_feature_bwd(const float* dphi, const float* z, void* dz, int dtype, int64_t rows, int ld, int nvalid, void* stream);
/* Feed-forward hidden backward, for h = dropout(relu(hpre)) of the training-mode forward (rf_dropout mask (p, seed, offset)):
 *   dh[e] = hpre[e] > 0 ? g[e] * keep(e) / (1 - p) : 0     (p = 0: no mask)   g, hpre fp32 [n]; dh of dtype [n]; 0 <= p < 1 */
int rf_relu_dropout_bwd(const float* g, const float* hpre, void* dh, int dtype, float p, uint64_t seed, uint64_t offset, int64_t n,
                        void* stream);

/* ---- backward pass of GraphTransformer and its block (csrc/backward.hip; model.py, rf.py:613-676) ---------------------------
 * Backward of the attention core, one entry point for rf_graph_attention (mask NULL, p = 0), rf_graph_attention_dropout (mask
 * NULL, p > 0) and rf_graph_attention_masked (mask, any p).  For a row (b, i) and head h, over the row's columns j (all of them,
 * or the mask's), with keep_j the forward's keep / drop decision of element [b, h, i, j] of the [B, H, L, L] map (seed, offset):
 *   s_j = scale q_i.(k_j + e_ij),  p = softmax(s),  pd_j = keep_j p_j / (1 - p_drop),  out_i = sum_j pd_j (v_j + e_ij)
 *   dp_j = keep_j / (1 - p_drop) g_i.(v_j + e_ij),   ds_j = p_j (dp_j - sum_l p_l dp_l)
 *   dq_i = scale sum_j ds_j (k_j + e_ij)             de_ij = pd_j g_i + scale ds_j q_i
 *   dk_j = scale sum_i ds_ij q_i                     dv_j = sum_i pd_ij g_i
 * q, k, v [B,L,H*d] and e [B,L,L,H*d] of dtype (the forward's operands: nothing of size L*L is saved, a block per row recomputes
 * its logits and probabilities); g fp32 [B,L,H*d] = d out.  Outputs: dq, dk, dv fp32 [B,L,H*d]; de [B,L,L,H*d] of dtype;
 * pd_map, ds_map fp32 [B,H,L,map_ld] (map_ld >= L).  The maps are fp32 in every build: dk and dv are sums of up to L of their
 * entries, taken by a second kernel in ascending row order (no atomics: the same bits run to run), and so carry no 16-bit
 * rounding; they are 2 / (H*d) of the bytes of e.  EVERY element of every output is written by the call -- nothing needs
 * pre-zeroing: de and both maps are exactly 0 at a masked column, the maps also in the pad columns [L, map_ld).
 * Under a mask the reads follow the row's degree (the forward's column compaction; k, v, e at a masked column are never read) and
 * an all-ones mask gives the NULL-mask call's bits.  A row with no edge attends uniformly with the constant logit 0 (the forward's
 * rule), which does not depend on q, k, e: dq_i = 0 and ds = 0 exactly, and de, dv receive the value path only, pd_j g_i with
 * p_j = 1 / L (k, v, e of the row are not read).  That is the derivative of the function the forward computes; the reference's
 * autograd would push a gradient through logits that its own -1e9 rounds away, and is not followed.
 * Accumulation: the per-channel dot products in fp32; the softmax normaliser, sum_l p_l dp_l, the sums over columns (dq) and over
 * rows (dk, dv) in fp64 (a row of two or three edges cancels in dp_j - sum_l p_l dp_l), each result rounded once to its type.
 * e is read twice per row (the second time from L2), de written once.
 * RF_EINVAL before any launch: a NULL tensor, p outside [0, 1), H*d > 256, d > 64 or not a power of two, map_ld < L, or
 * (2*H*L + 2*L + 520) * 4 bytes of LDS > 64 KB (twice the forward's logits, plus the column list, its inverse and the partial
 * dq: at H = 4, L <= 1586; at H = 8, L <= 881). */
int rf_graph_attention_bwd(const void* q, const void* k, const void* v, const void* e, int dtype, const uint8_t* mask,
                           const float* g, float* dq, float* dk, float* dv, void* de, float* pd_map, float* ds_map, int64_t map_ld,
                           int B, int L, int H, int d, float scale, float p, uint64_t seed, uint64_t offset, void* stream);
/* ELU backward from the activation's value, for y = x + ELU(z) (GraphTransformerBlock's tail, rf.py:674-676; x NULL: y = ELU(z)):
 *   a = y[e] - x[e],  da[e] = g[e] * (a > 0 ? 1 : a + 1)       g, y, x fp32 [n]; da of dtype [n]
 * (rf_instnorm_bwd applies the same factor inside its own passes; no stand-alone kernel had it). */
int rf_elu_bwd(const float* g, const float* y, const float* x, void* da, int dtype, int64_t n, void* stream);

/* ---- backward pass of PositionWiseWeightFactor and of the structure track's node input (csrc/backward.hip; model.py
 * PositionWiseWeightFactor, _node_input; rf.py:205-217, 715-724) --------------------------------------------------------------
 * Backward of rf_poswise, with rf_poswise's addressing (rf_version >= 15): q0 [B,L,H*dlen] of q0_dtype (q0_ld between rows), k
 * rows [B,N,L,*] of dtype (k_ld between rows, head h at column k_col0 + h*k_hstride, dlen columns).  Per (b, l, h), over the MSA
 * depth n, with keep_n the keep / drop decision of element [b, n, h, l] of rf_dropout's mask (p, seed, offset) over the
 * contiguous [B,N,H,L] weights (p = 0: no dropout):
 *   w_n = softmax_n(scale q0_h . k_{n,h}),   wd_n = w_n keep_n / (1 - p)
 *   dw_n = keep_n / (1 - p) (dw[b,n,h,l] + k_n . ds[b,l,:])        dw fp32 [B,N,H,L] = the gradient of the (dropped) weights
 *   dlogit_n = w_n (dw_n - sum_m w_m dw_m)
 *   dq0[b,l,h,:]   = scale sum_n dlogit_n k_{n,h,:}                 fp32 [B,L,H*dlen], contiguous
 *   dk[b,n,l,h,:]  = scale dlogit_n q0_h + wd_n ds[b,l,:]           of dk_dtype (fp32 or the 16-bit type): rows [B,N,L,*] of
 *                                                                   dk_ld, head h at column dk_col0 + h*dk_hstride
 * ds fp32 [B,L,*] (ds_ld between rows) is the gradient of s[b,l,:] = sum_n wd_n k_n, rf_weighted_msa_sum fused behind the
 * weights: the collapsed one-head form only (H == 1, dlen = the whole row; k_hstride and dk_hstride are not used).  dw or ds
 * may be NULL (not both); with ds == NULL the second term of dk is absent.  The collapsed form with H > 1 is NOT supported with
 * ds (RF_EINVAL: dk would be a sum over heads); without ds any H, k_hstride == 0 included, is taken as the addressing says.
 * Nothing of the forward is saved but its inputs: a block per (b, l) recomputes the logits and w.  to_k's bias is constant over
 * n, drops out of the softmax, has gradient zero and never reaches this kernel.
 * k is read twice (the second time from L2), dk written once; 16-byte accesses when dlen % 8 == 0, every leading dimension,
 * column offset and head stride is a multiple of 8 and the tensors are 16-byte aligned, a scalar path otherwise.
 * Accumulation: the dot products in fp32; the softmax normaliser, sum_m w_m dw_m (N = 2 or 3 cancels in dw_n - sum) and the sums
 * over n into dq0 in fp64; each result rounded once.  No atomics: the same bits run to run.  N == 1: dlogit = 0 and dq0 = 0
 * exactly, dk = wd ds alone.  EVERY element of dq0 and of the addressed columns of dk is written by the call.
 * RF_EINVAL before any launch: q0, k, dq0 or dk NULL, dw and ds both NULL, ds with H != 1, p outside [0, 1), or
 * (2*N*H + 512) * 4 bytes of LDS > 64 KB (logits and dlogit, plus the reduction scratch of dq0). */
int rf_poswise_bwd(const void* q0, int q0_dtype, int64_t q0_ld, const void* k, int dtype, int64_t k_ld, int k_col0, int k_hstride,
                   int dlen, const float* dw, const float* ds, int64_t ds_ld, float* dq0, void* dk, int dk_dtype, int64_t dk_ld,
                   int dk_col0, int dk_hstride, int B, int N, int L, int H, float scale, float p, uint64_t seed, uint64_t offset,
                   void* stream);

/* ---- backward pass of MsaUpdateWithPairAndCoord (csrc/backward.hip; structure.py, rf.py:865-920) ---------------------------
 * Backward of rf_dist_masked_attention (rf_version >= 16).  Per (b, h, i), over the columns j, with the forward's
 *   logit_j = q_i . k_j + (|CA_i - CA_j| < bins[h] ? 0 : -1e9),   p = softmax_j(logit):
 *   ds_j = p_j (datt_j - sum_l p_l datt_l)        datt fp32 [B,H,L,L] = the gradient of the probabilities
 *   dq[b,i,h,:] = sum_j ds_ij k[b,j,h,:]          dk[b,j,h,:] = sum_i ds_ij q[b,i,h,:]
 * q (pre-scaled, as the forward sees it: the caller multiplies dq by its scale) and k: fp32 [B,L,H*d]; xyz fp32 [B,L,3,3];
 * bins fp32 [H].  Outputs: dq, dk fp32 [B,L,H*d]; ds_map fp32 [B,H,L,L], the workspace the second kernel sums dk from, which
 * holds ds on return.  EVERY element of the three is written by the call.  xyz receives no gradient: the mask is piecewise
 * constant.  Nothing of the forward is saved but its inputs: a block per (b, i) recomputes the row in fp32 (the stored map is
 * 16-bit and is not read) and takes the distance test with the forward's own fp32 expression, so both masks agree bit for bit.
 * A masked entry has p = 0 exactly (exp(-1e9 - max) = 0) and so ds = 0 exactly; a residue out of every other residue's range
 * has p = 1 on itself, and its rows of dq and dk are exactly 0, as are all of dq and dk at L == 1.
 * Accumulation: the dot products q.k in fp32 in the forward's order; the softmax normaliser, sum_l p_l datt_l and the sums over
 * j (dq) and over i (dk) in fp64, each result rounded once.  No atomics: the same bits run to run.  datt is read twice per row
 * (the second time from cache) so that the LDS need stays the forward's.
 * RF_EINVAL before any launch: a NULL tensor, a size <= 0, or H * L * 4 bytes of LDS > 64 KB (the forward's own limit; any d). */
int rf_dist_masked_attention_bwd(const float* q, const float* k, const float* xyz, const float* bins, const float* datt,
                                 float* dq, float* dk, float* ds_map, int B, int L, int H, int d, void* stream);

/* ---- backward pass of SoftTiedAttentionOverResidues (csrc/backward.hip; model.py, rf.py:220-267) ---------------------------
 * Backward of the tied attention's softmax and of its symmetrised map (rf_version >= 17).  Per (b, h, i), over the columns j:
 *   p = softmax_j(logits[b,h,i,:]),   dp_j = dp[b,h,i,j] + (g_sym[b,i,j,h] + g_sym[b,j,i,h]) / 2,
 *   ds[b,h,i,j] = p_j (dp_j - sum_l p_l dp_l)
 * logits, dp (the value-path part of the probabilities' gradient) and ds: fp32 [B,H,L,L], contiguous; g_sym: fp32 [B,L,L,H],
 * contiguous, the gradient of sym[b,i,j,h] = (p[b,h,i,j] + p[b,h,j,i]) / 2, or NULL (no second term).  p_h16 and ds_h16, each
 * may be NULL: copies of p and of ds in the build's 16-bit type, [B,H,L,ld] with ld >= L elements between rows (ld a multiple of
 * 8, else RF_EALIGN; ld is not read when both are NULL); their columns [L, ld) are written as zeros, the convention of
 * rf_tied_softmax_ld, so that both are legal 16-bit rf_gemm operands with K = ld at any L.
 * Nothing of the forward is saved but the fp32 logits: p is recomputed in fp32 with the row maximum subtracted; the normaliser
 * and sum_l p_l dp_l are fp64 sums, each ds rounded once.  L == 1: ds = 0 exactly.  Any L >= 1 and any H >= 1; EVERY element
 * of every output handed in is written (the pads included), nothing else is; no atomics: the same bits run to run.
 * A block takes up to 16 query rows of one sample with all heads and stages the half-sum of g_sym for them in LDS (at most
 * 64 KB; one row with all heads that does not fit, H * (L | 1) * 4 bytes > 64 KB, reads g_sym from memory instead).
 * RF_EINVAL before any launch: logits, dp or ds NULL, a size <= 0, L * H >= 2^27, a 16-bit copy with ld < L. */
int rf_tied_softmax_bwd(const float* logits, const float* dp, const float* g_sym, float* ds, void* p_h16, void* ds_h16, int64_t ld,
                        int B, int H, int L, void* stream);
/* Backward of rf_scale_rows with a factor, y[r,:] = alpha w[r] x[r,:] (rf_version >= 17), over rows r = (t, h), t < tokens,
 * h < H, of D columns.  Row (t, h) of x starts at element t * x_ld + h * x_hs, and likewise for gy (the gradient of y) and dx;
 * x, gy and dx are fp32 or the build's 16-bit type, each with its own dtype code; w and dw are fp32 [tokens * H], contiguous:
 *   dx[r,:] = alpha w[r] gy[r,:]          dw[r] = alpha sum_c gy[r,c] x[r,c]      (an fp64 sum, rounded once)
 * So the q block of a [.., 3 D] projection buffer is walked in place with ld = 3 D, hs = d_head, D = d_head, as rf_poswise does.
 * dx or dw may be NULL (not both); dx may be gy itself (same dtype and strides).  EVERY addressed element of dx and every
 * element of dw is written, nothing else is; no atomics: the same bits run to run.
 * RF_EINVAL before any launch: x, gy or w NULL, dx and dw both NULL, a size <= 0, a negative stride, tokens * H >= 2^34. */
int rf_scale_rows_bwd(const void* x, int x_dtype, int64_t x_ld, int64_t x_hs, const void* gy, int gy_dtype, int64_t gy_ld,
                      int64_t gy_hs, const float* w, float alpha, void* dx, int dx_dtype, int64_t dx_ld, int64_t dx_hs, float* dw,
                      int64_t tokens, int H, int D, void* stream);

/* ---- backward pass of MsaUpdateWithPair (csrc/backward.hip; model.py, rf.py:559-610) ----------------------------------------
 * Backward of the batched per-(layer, head) softmax of the shared front (rf_version >= 18).  logits: fp32 [B,L,L,NZ], what
 * rf_softmax_batched read (after the logit dropout when there was one), map z = layer * H + head innermost; datt: fp32
 * [NZ,B,L,datt_ld], the gradient of the maps, datt_ld >= L elements between rows (columns j >= L are neither read nor written);
 * dz: fp32 [B,L,L,NZ], the logits' gradient:
 *   p = softmax_j(logits[b,i,:,z]),   dz[b,i,j,z] = p_j (datt[z,b,i,j] - sum_l p_l datt[z,b,i,l])
 * dz_h16, may be NULL: the same gradient in the build's 16-bit type, [B,L,L,nz_pad] with nz_pad >= NZ a multiple of 8 and exact
 * zeros in the columns [NZ, nz_pad): the dy operand of rf_conv_wgrad, whose Co must be a multiple of 8 (nz_pad is not read
 * when dz_h16 is NULL).  p is recomputed in fp32 with the row maximum subtracted; the normaliser and sum_l p_l datt_l are fp64
 * sums, each dz rounded once.  L == 1: dz = 0 exactly.  A block owns one (b, i), whose NZ rows are one contiguous slab of L * NZ
 * floats of logits and of dz; it holds the slab in NZ * (L | 1) * 4 bytes of LDS.  EVERY element of dz (and of dz_h16) is
 * written, nothing else is; no atomics: the same bits run to run.
 * RF_EINVAL before any launch: logits, datt or dz NULL, a size <= 0, datt_ld < L, with dz_h16 nz_pad < NZ or nz_pad % 8, or a
 * slab beyond 160 KB of LDS (L * NZ of about 40900). */
int rf_pair_softmax_bwd(const float* logits, const float* datt, int64_t datt_ld, float* dz, void* dz_h16, int nz_pad, int B, int L,
                        int NZ, void* stream);
/* Backward of z = rf_sym_layernorm(pair) . w^T (rf_version >= 18): pair fp32 [B,L,L,D]; w fp32 [NZ,D], the projection with the
 * LayerNorm's gamma folded in; dz fp32 [B,L,L,NZ]; dpair fp32 [B,L,L,D].  With s = (pair_ij + pair_ji) / 2, xhat and rstd its
 * LayerNorm statistics (two-pass fp32, as the forward takes them) and g = (dz_ij + dz_ji) . w:
 *   dpair_ij = dpair_ji = rstd / 2 * (g - mean g - xhat mean(g xhat))
 * One wave per unordered pair i <= j: both rows of pair and of dz are read once, both rows of dpair are written once (the
 * diagonal once), bit for bit the same; g lives in registers (NZ fp32 FMAs per element from w in LDS; from memory when w exceeds
 * 64 KB), the two means are fp64 sums.  EVERY element of dpair is written; no atomics: the same bits run to run.
 * RF_EINVAL before any launch: a NULL tensor, a size <= 0, D % 4, D > 1024 or NZ > 64; RF_EALIGN: pair, w or dpair not 16-byte
 * aligned. */
int rf_sym_layernorm_bwd(const float* pair, const float* dz, const float* w, float* dpair, int B, int L, int D, int NZ, float eps,
                         void* stream);

/* ---- backward pass of MsaEmbedding and PairEmbedding (csrc/backward.hip; model.py, rf.py:106-181) ---------------------------
 * Gradient of an embedding table (rf_version >= 21).  idx: int64 [rows], the token of each row; g: fp32 [rows, D], contiguous,
 * the gradient of dropout(table[idx] + ...) + query_enc; dtable: fp32 [V, D]:
 *   dtable[t, c] = sum over the rows r with idx[r] == t of keep(r, c) / (1 - p) * g[r, c]
 * with keep the keep / drop decision of element r * D + c of rf_dropout's mask (p, seed, offset) over the contiguous [rows, D]
 * tensor, replayed inside the kernel; the term is rf_dropout's own fp32 product g * (1 / (1 - p)).  p = 0: no dropout (seed and
 * offset are not read).  dq, may be NULL: fp32 [2, D], the gradient of the two query-encoding rows from the UNMASKED g (the
 * reference adds query_enc behind the dropout): with row r = (b, n, l) of [.., N, L], n = (r / L) % N,
 *   dq[0, c] = sum over the rows with n == 0 of g[r, c],   dq[1, c] = sum over the rows with n >= 1 of g[r, c]
 * The pair side calls it with rows = B * L, idx = seq and N = 1 (N and L are read for dq only).
 * Accumulation: every sum in fp64, rounded once.  A wave owns 256 consecutive rows and 64 channels and keeps its [V, 64] sums in
 * LDS; a block of 4, 2 or 1 waves (the most whose sums fit 64 KB) writes one fp64 partial [V + 2, D] to the workspace, and a
 * second launch adds the partials in block order: no atomics, the same bits run to run.  g is read once.  A table row whose
 * index never occurs is written as exact zeros, as is dq[1] at N == 1; a row whose index lies outside [0, V) adds to dq only.
 * EVERY element of dtable (and of dq) is written, nothing else is.  Workspace (8-byte aligned): rf_embedding_bwd_ws_bytes bytes
 * (0: an empty or refused problem).
 * RF_EINVAL before any launch: idx, g, dtable or the workspace NULL, a size <= 0, p outside [0, 1), a workspace too small, or
 * (V + 2) * 512 bytes of LDS > 64 KB (V > 126). */
int64_t rf_embedding_bwd_ws_bytes(int64_t rows, int D, int V);
int rf_embedding_bwd(const int64_t* idx, const float* g, float* dtable, float* dq, int64_t rows, int D, int V, int N, int L, float p,
                     uint64_t seed, uint64_t offset, void* workspace, int64_t ws_bytes, void* stream);
/* The sums of a pair-shaped gradient over each picture axis, and the gradients of rf_pair_embed's separation column and bias
 * (rf_version >= 21).  g: fp32 [B,L,L,D], contiguous; aa_idx: int64 [B,L]:
 *   rows[b,i,c] = sum_j g[b,i,j,c]            cols[b,j,c] = sum_i g[b,i,j,c]            (fp32 [B,L,D] each)
 *   dsep[c]  = sum_{b,i,j} g[b,i,j,c] * logf((float)(|aa_idx[b,i] - aa_idx[b,j]| + 1))   (fp32 [D]; the forward's own expression)
 *   dbias[c] = sum_{b,i,j} g[b,i,j,c]                                                    (fp32 [D])
 * By linearity these are what every feature tiled along one axis of a pair picture needs for its gradient.
 * Accumulation: every sum in fp64 (the product with the fp32 separation is exact there), rounded once.  g is read once: a block
 * takes 16 rows x 64 columns of one sample and 64 channels, writes the column sums of its 16 rows and the row sums of its 64
 * columns as fp64 partials, and a second launch adds the row tiles' (column tiles', blocks') partials in ascending order: no
 * atomics, the same bits run to run.  L == 1: dsep = 0 exactly.  EVERY element of the four outputs is written, nothing else is.
 * Workspace (8-byte aligned): rf_pair_axis_sums_ws_bytes bytes.  The LDS need is 40 KB at every shape.
 * RF_EINVAL before any launch: a NULL tensor or workspace, a size <= 0, a workspace too small, or
 * B * ceil(L/16) * ceil(L/64) >= 2^31. */
int64_t rf_pair_axis_sums_ws_bytes(int B, int L, int D);
int rf_pair_axis_sums(const float* g, const int64_t* aa_idx, float* rows, float* cols, float* dsep, float* dbias, int B, int L,
                      int D, void* workspace, int64_t ws_bytes, void* stream);

/* ---- backward pass of the SE(3) node layers and of the graph attention (csrc/se3.hip; structure.py GNormBias, G1x1SE3,
 * GAttentiveSelfInt, GMABSE3; ea/modules.py:328-473, 683-774) ------------------------------------------------------------------
 * rf_version >= 22.  All tensors are fp32 in both builds (the structure track is fp32 in every compute mode).  Nothing of the
 * forward is saved but its inputs.  The fp32 operands are widened to fp64, every sum (dot products, softmax normalisers, the sums
 * over edges, channels and nodes) is an fp64 sum, and each result is rounded once.  No atomics: the same bits run to run.  EVERY
 * addressed output element is written by the call.  The two contractions that are left (G1x1SE3's weight gradient and the Linear
 * inside GAttentiveSelfInt) run on rf_gemm (RF_F32) and rf_conv_wgrad (RF_F32), which take any channel count in fp32.
 *
 * Backward of rf_se3_attention, with the forward's addressing: the same per-edge k0, k1, v0, v1, per-node q0, q1, dense eid map,
 * heads, mk*, mv*, V, L and the same limit L <= 1024.  g0 / g1: the gradient of out0 / out1, rows g0_ld / g1_ld floats apart
 * (0 = packed: mv0 / 3*mv1), so that it can be the leading channels of the GCat buffer's gradient.  Per (dst node, head), over the
 * node's incoming edges e in the forward's order, on this head's channels of both degrees:
 *   p_e  = softmax_e(<k_e, q_node> / sqrt(mk0 + 3 mk1))        recomputed in fp64, maximum subtracted
 *   dv_e = p_e g_node          dp_e = <v_e, g_node>          S = sum_e p_e dp_e          dl_e = p_e (dp_e - S)
 *   dk_e = dl_e q_node / sqrt(nfeat)                          dq_node = sum_e dl_e k_e / sqrt(nfeat)
 * dk0, dk1, dv0, dv1 are per-edge like k and v, dq0, dq1 per-node like q (packed).  An edge has one dst: one wave owns each
 * (edge, head) slice of dk / dv and each (node, head) slice of dq.  A node of in-degree 0 gets dq exactly 0; a node of in-degree
 * 1 gets dk exactly 0 on that edge, dq exactly 0 and dv equal to g bit for bit.  Edge rows the eid map does not name (at or above
 * the edge count) are not written.  A degree with mk = 0 (mv = 0) takes NULL pointers.
 * RF_EINVAL before any launch: a NULL tensor of a present degree, a size <= 0, L > 1024, V % L != 0, a channel count that
 * `heads` does not divide, a g_ld below its row. */
int rf_se3_attention_bwd(const float* k0, const float* k1, const float* q0, const float* q1, const float* v0, const float* v1,
                         const int32_t* eid, const float* g0, const float* g1, int64_t g0_ld, int64_t g1_ld, float* dk0, float* dk1,
                         float* dq0, float* dq1, float* dv0, float* dv1, int heads, int mk0, int mk1, int mv0, int mv1, int V, int L,
                         void* stream);
/* Backward of rf_se3_norm_bias.  v, g (the gradient of y), dv: [V, m, 2 deg + 1]; bias, dbias: [m].  With n = max(|v|, 1e-12),
 * t = relu(n + b_c), y = t v / n: where n + b_c > 0 (the forward's own fp32 test, so that both take the same side of the kink)
 *   dv = (t / n) g + (1 / n - t / n^2) (<v, g> / n) v        (the second term absent where |v| < 1e-12: n is a constant there)
 *   dbias[c] = sum over the nodes of <v, g> / n
 * and elsewhere dv and the node's term of dbias are exactly 0.  A thread owns one (node, channel); the terms of dbias go to the
 * workspace (fp64, rf_se3_norm_bias_bwd_ws_bytes bytes, 8-byte aligned; 0 for an empty problem) and one block per channel adds
 * them in a fixed order.  RF_EINVAL before any launch: a NULL tensor or workspace, a size <= 0, a workspace too small. */
int64_t rf_se3_norm_bias_bwd_ws_bytes(int64_t V, int m, int deg);
int rf_se3_norm_bias_bwd(const float* v, const float* bias, const float* g, float* dv, float* dbias, int64_t V, int m, int deg,
                         void* workspace, int64_t ws_bytes, void* stream);
/* Backward of rf_se3_gram.  v, dv: [V, m, 2 deg + 1]; ds: [V, m*m], the gradient of s:
 *   dv_a (+)= sum_b (ds[a,b] + ds[b,a]) [|<v_a, v_b>| >= 1e-12] v_b
 * The bracket is the clamp's derivative, decided by the forward's own fp32 product.  accumulate != 0: added (in fp64, one rounding)
 * to what dv holds -- GAttentiveSelfInt reads v twice, and dv already carries rf_se3_attn_apply_bwd's dx.  A thread owns one
 * (node, a).  deg is 0 or 1.  RF_EINVAL before any launch: a NULL tensor, a size <= 0, deg outside [0, 1]. */
int rf_se3_gram_bwd(const float* v, const float* ds, float* dv, int accumulate, int64_t V, int m, int deg, void* stream);
/* Backward of rf_se3_attn_apply.  att, datt: [V, m_out*m_in]; x, dx: [V, m_in, 2 deg + 1]; g: [V, m_out, 2 deg + 1], the gradient
 * of y.  Per node, with p = softmax_m(att[n,o,:]) recomputed in fp64:
 *   datt[n,o,m] = p_m (<g[n,o,:], x[n,m,:]> - sum_l p_l <g[n,o,:], x[n,l,:]>)          dx[n,m,:] = sum_o p[o,m] g[n,o,:]
 * A block owns one node and keeps its probabilities in m_out * m_in * 8 bytes of LDS: the sum over o never leaves the block.
 * RF_EINVAL before any launch: a NULL tensor, a size <= 0, deg outside [0, 1], more than 64 KB of LDS (m_out * m_in > 8192). */
int rf_se3_attn_apply_bwd(const float* att, const float* x, const float* g, float* datt, float* dx, int64_t V, int m_out, int m_in,
                          int deg, void* stream);
/* Backward of rf_layernorm followed by act = RF_ACT_LEAKY (slope 0.01) or RF_ACT_NONE, at ANY D >= 1 (rf_layernorm_bwd stops at
 * 1024; GAttentiveSelfInt normalises m_in^2 values: 361, 2304).  x (the forward's input), g (the gradient of the activation's
 * output), dx: fp32 [rows, D], contiguous; gamma, beta, dgamma, dbeta: fp32 [D].  Mean and rstd are recomputed two-pass in fp64:
 *   ge = g * (act == RF_ACT_LEAKY && gamma xhat + beta <= 0 ? 0.01 : 1)       (the gate from these fp64 statistics, not from the
 *                                                                               forward's fp32 output: an output within fp32
 *                                                                               rounding distance of 0 may take the other side)
 *   dx = rstd * (ge gamma - mean(ge gamma) - xhat * mean(ge gamma xhat))       dgamma[c] = sum_rows ge xhat,  dbeta[c] = sum_rows ge
 * A block per row with a strided loop writes dx and the row's statistics; a thread per column sums chunks of 64 rows into fp64
 * partials, which a last launch adds in chunk order.  dgamma or dbeta may be NULL (both: dx only).  Workspace (8-byte aligned):
 * rf_layernorm_act_bwd_ws_bytes bytes (0 for an empty problem).
 * RF_EINVAL before any launch: a NULL tensor or workspace, a size <= 0, another activation, rows > 64 * 65535, a workspace too
 * small. */
int64_t rf_layernorm_act_bwd_ws_bytes(int64_t rows, int D);
int rf_layernorm_act_bwd(const float* x, const float* g, const float* gamma, const float* beta, float eps, int act, float* dx,
                         float* dgamma, float* dbeta, int64_t rows, int D, void* workspace, int64_t ws_bytes, void* stream);

/* Library self-description */
/* Timing experiments only: when buf is non-null every bf16 rf_gemm workgroup records 8 x uint64 phase stamps into it. */
int rf_debug_gemm_stamps(void* buf);
int rf_debug_gemm_fast_stamps(void* buf);

int rf_version(void);
const char* rf_build_info(void);
int rf_h16_dtype(void); /* RF_BF16 (librfmi.so) or RF_F16 (librfmi_f16.so) */

#ifdef __cplusplus
}
#endif
#endif /* RFMI_H */
