// K1L -- SCDM additive cross-attention for sentences of up to 128 words (gfx950, MI355X).
//
// Same mathematics as K1 / K1g (scdm_attn.hip, header comment), which stop at 32 words:
//     e[b,t,n] = sum_k w[k] tanh(a[b,t,k] + s[b,n,k]);  P = softmax_n(e);  C = P @ V
//     out = r * sigmoid(P @ VW + gbias)                                   (gate-fused form, V = VW)
// with tanh(a+s) = 1 - 2/(Ea*Es + 1), Ea = exp(2a), Es = exp(2s), a and s clamped to +-40 before the exponential (Ea*Es may overflow
// to +inf or underflow to 0 -- the reciprocal is then 0 or 1 -- but is never NaN); the constant sum_k w[k] cancels in the softmax, so
// e'[t,n] = -2 sum_k w[k] / (Ea*Es + 1) is what is accumulated.  Operands beyond +-40 themselves take the sum form (rcp_sum_form below), so that
// a large a and a large s of opposite sign still score tanh of their true sum.
//
// K1 keeps Es[b] of ALL words in LDS and one accumulator per word in registers; neither scales past 32 words.  Here the words are
// walked in chunks of kNC = 16:
//   forward (one launch): workgroup = (b, 32 clip rows), 8 waves x 4 rows.  The rows stay in registers (H <= 1024: 4 float4 per lane
//     and row).  Per word chunk: Es rows of the chunk -> LDS [16][HP] (64 KiB at H = 1024), k swept in 256-column chunks with the 4 rows
//     blocked in registers (16 accumulators per row), wave transpose-sum, raw scores -> LDS [32][roundup(N,16)].  After the last chunk:
//     softmax over the N scores of each row (P -> LDS and HBM), then C = P @ V with one column pair per thread and all 32 rows blocked
//     in registers (V[b] is read once per workgroup), gate epilogue where fused.
//   backward (five launches: ds runs as two that split the workgroups between the product and the sum form, no exchange between workgroups, every large output written exactly once, no float atomics on them):
//     rows : (b, 32 rows)  [gate: z = P VW + gbias, dr = dout sig(z), dz = dout r sig(z)(1 - sig(z)) -> workspace]
//                          dP = dz V^T, de = P (dP - <P,dP>) -> workspace                 (V chunks staged in LDS)
//     da   : (b, 16 rows)  da[t,k] = 4 w[k] sum_n de[t,n] q,  q = r(1-r), r = 1/(Ea Es + 1)    (the forward's score loop with de as weights)
//     ds   : (b, 256 columns, 16 words) sweeping all T rows: ds[n,k] = 4 w[k] sum_t de[t,n] q; dw[k] += -2 sum_{t,n} de[t,n] r  (atomics: dw only)
//     dv   : (b, 256 columns, 16 words) sweeping all T rows: dV[n,j] = sum_t P[t,n] dz[t,j];   dgbias[j] += sum_t dz[t,j]     (atomics: dgbias only)
//   da and ds both recompute r: da wants the words innermost, ds the rows, and a sum held across the other loop would need either
//   N x 4 or T x 4 registers per lane or an exchange through memory.
#include "tsg_common.h"
#include <initializer_list>
#include <type_traits>

namespace tsg {
namespace {

constexpr int kLongMaxWords = 128;
constexpr int kLongMaxH = 1024;               // a wave keeps its clip rows in registers: 4 float4 per lane and row
constexpr int kLongMaxDs = 1024;              // ... and the rows kernel its dz rows
constexpr int kNC = 16;                       // words per chunk
constexpr int kRowThreads = 512;              // row-tiled kernels: 8 waves x kRowR rows
constexpr int kRowWaves = kRowThreads / kWave;
constexpr int kRowR = 4;
constexpr int kRowTT = kRowWaves * kRowR;     // 32 rows per workgroup
constexpr int kDaR = 2;                       // the da kernel: 2 rows per wave (with 4 the 64 da sums + 64 row registers spilled)
constexpr int kDaTT = kRowWaves * kDaR;
constexpr int kColThreads = 256;              // column-sliced kernels: 4 waves share the T rows
constexpr int kColWaves = kColThreads / kWave;
constexpr float kClamp = 40.0f;

__host__ __device__ __forceinline__ int roundup256(int x) { return (x + 255) & ~255; }
__host__ __device__ __forceinline__ int roundup16(int x) { return (x + 15) & ~15; }

__device__ __forceinline__ int wave_id() { return __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)); }

__device__ __forceinline__ float4 exp2x4(float4 v) {     // exp(2 v), v clamped to +-kClamp
  return make_float4(fast_exp2(clampf(v.x, -kClamp, kClamp) * k2Log2e), fast_exp2(clampf(v.y, -kClamp, kClamp) * k2Log2e),
                     fast_exp2(clampf(v.z, -kClamp, kClamp) * k2Log2e), fast_exp2(clampf(v.w, -kClamp, kClamp) * k2Log2e));
}
// The product form needs exp(2a) and exp(2s) each inside fp32's range, hence the separate clamps -- exact only while |a| and |s| stay within
// kClamp (beyond it a = 90, s = -90.3 would score as tanh(0)).  Where a wave meets such an operand (never with trained activations; the
// saturation tests do it on purpose) it takes the sum form for that chunk: r = 1 / (exp(2 clamp(a + s)) + 1), one more transcendental per element.
__device__ __forceinline__ bool beyond_clamp(float4 v) {
  return fmaxf(fmaxf(fabsf(v.x), fabsf(v.y)), fmaxf(fabsf(v.z), fabsf(v.w))) > kClamp;
}
__device__ __forceinline__ bool wave_any(bool p) { return __builtin_amdgcn_ballot_w64(p) != 0; }
__device__ __forceinline__ float rcp_sum_form(float a, float s) { return fast_rcp(fast_exp2(clampf(a + s, -kClamp, kClamp) * k2Log2e) + 1.f); }
constexpr int kMaxChunks = kLongMaxWords / kNC;

__device__ __forceinline__ float sigmoidf(float x) { return fast_rcp(1.f + fast_exp2(-x * kLog2e)); }

// Sum 16 per-lane partials over the 64 lanes (the scheme of scdm_attn.hip's wave_transpose_sum): v_permlane32_swap folds the wave halves
// of two values at once, v_permlane16_swap the 16-lane rows of each half, 4 DPP steps finish inside a row.  Afterwards register j,
// 16-lane row q holds the total for value 4j + {0,2,1,3}[q].
__device__ __forceinline__ void wave_transpose_sum16(const float (&v)[kNC], float (&z)[kNC / 4]) {
  float h[kNC / 2];
#pragma unroll
  for (int i = 0; i < kNC / 2; ++i) {
    const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(v[2 * i]), __float_as_uint(v[2 * i + 1]), false, false);
    h[i] = __uint_as_float(r[0]) + __uint_as_float(r[1]);
  }
#pragma unroll
  for (int j = 0; j < kNC / 4; ++j) {
    const auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(h[2 * j]), __float_as_uint(h[2 * j + 1]), false, false);
    float t = __uint_as_float(r[0]) + __uint_as_float(r[1]);
    t += dpp_mov<0xB1>(t);    // quad_perm [1,0,3,2]
    t += dpp_mov<0x4E>(t);    // quad_perm [2,3,0,1]
    t += dpp_mov<0x141>(t);   // row_half_mirror
    t += dpp_mov<0x140>(t);   // row_mirror
    z[j] = t;
  }
}
// ... and the 16 totals of one tile row into LDS (dst = the row's slot of word c0)
__device__ __forceinline__ void store_chunk_sums(const float (&v)[kNC], float* dst, int lane) {
  float z[kNC / 4];
  wave_transpose_sum16(v, z);
  const int q = lane >> 4, word = ((q & 1) << 1) | (q >> 1);
  if ((lane & 15) == 0) {
#pragma unroll
    for (int j = 0; j < kNC / 4; ++j) dst[4 * j + word] = z[j];
  }
}

// Words [c0, c0 + kNC) of src[b] ([N][W] storage) -> LDS [kNC][WP] fp32, as exp(2 x) (EXP) or as they are; zero beyond N and W.
// (Zero Es: r = 1 for a padded word or column -- the column's weight is 0 and the word is masked in the softmax.)
template <bool EXP, typename ST>
__device__ __forceinline__ void stage_words(float* __restrict__ dst, const ST* __restrict__ srcb, int c0, int N, int W, int WP, int tid,
                                            int* big = nullptr) {        // *big = 1 when a staged value lies beyond the clamp (EXP only)
  const int wp4 = WP / 4, total4 = kNC * wp4;
  constexpr int PU = 8;                              // every load of a round issued before the first exp
  for (int base = tid; base < total4; base += PU * kRowThreads) {
    float4 v[PU];
    bool ok[PU];
#pragma unroll
    for (int u = 0; u < PU; ++u) {
      const int idx = base + u * kRowThreads;
      const int n = c0 + idx / wp4, k = (idx % wp4) * 4;
      ok[u] = idx < total4 && n < N && k < W;
      v[u] = ok[u] ? ld4(srcb + (size_t)n * W + k) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
#pragma unroll
    for (int u = 0; u < PU; ++u) {
      const int idx = base + u * kRowThreads;
      if (idx < total4) {
        float4 e = EXP ? exp2x4(v[u]) : v[u];
        if (!ok[u]) e = make_float4(0.f, 0.f, 0.f, 0.f);
        if (EXP && big && beyond_clamp(v[u])) *big = 1;
        *reinterpret_cast<float4*>(dst + (idx / wp4) * WP + (idx % wp4) * 4) = e;
      }
    }
  }
}

// ------------------------------------------------------------------------------------------
// forward
// ------------------------------------------------------------------------------------------
// One 256-column step of the score loop for the wave's R rows and the chunk's 16 words: acc[r][n] += sum_c w2[c] / (Ea[r][c] Es[n][c] + 1).
// Words in pairs with the next pair's Es float4s in flight; the sched_barrier keeps the compiler from hoisting every product ahead of the
// first reciprocal (the register cost of that is what spilled in K1).
template <int R>
__device__ __forceinline__ void long_score_step(const float (&Ea)[R][4], const float* __restrict__ esp, int HP, const float (&w2)[4],
                                                float (&acc)[R][kNC]) {
  float4 cur[2], nxt[2];
  cur[0] = *reinterpret_cast<const float4*>(esp);
  cur[1] = *reinterpret_cast<const float4*>(esp + HP);
#pragma unroll
  for (int n0 = 0; n0 < kNC; n0 += 2) {
    if (n0 + 2 < kNC) {
      nxt[0] = *reinterpret_cast<const float4*>(esp + (n0 + 2) * HP);
      nxt[1] = *reinterpret_cast<const float4*>(esp + (n0 + 3) * HP);
    }
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const float e4[4] = {cur[u].x, cur[u].y, cur[u].z, cur[u].w};
#pragma unroll
      for (int r = 0; r < R; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[r][n0 + u] = fmaf(w2[c], fast_rcp(fmaf(Ea[r][c], e4[c], 1.f)), acc[r][n0 + u]);
    }
    __builtin_amdgcn_sched_barrier(0);
    cur[0] = nxt[0];
    cur[1] = nxt[1];
  }
}

// The scores of one word chunk for a wave's kRowR rows in the sum form (see rcp_sum_form): a + s first (both from L2), then one exponential;
// word by word, every total straight into the tile's score rows.  Not inlined: it is the rare path.
template <typename ST>
__device__ __noinline__ void fwd_chunk_sum_form(const ST* __restrict__ ab, const ST* __restrict__ sb, const float* Wl, float* sc, int t_first, int T,
                                                int N, int H, int HP, int SP, int c0, int lane) {
#pragma unroll 1
  for (int n = 0; n < kNC; ++n) {
    float part[kRowR];
#pragma unroll
    for (int r = 0; r < kRowR; ++r) part[r] = 0.f;
#pragma unroll 1
    for (int k = lane * 4; k < HP; k += 256) {
      const float4 wq = *reinterpret_cast<const float4*>(Wl + k);
      const float4 sv = (k < H && c0 + n < N) ? ld4(sb + (size_t)(c0 + n) * H + k) : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
      for (int r = 0; r < kRowR; ++r) {
        const int t = t_first + r;
        const float4 v = k < H ? ld4(ab + (size_t)(t < T ? t : T - 1) * H + k) : make_float4(0.f, 0.f, 0.f, 0.f);
        part[r] = fmaf(wq.x, rcp_sum_form(v.x, sv.x), part[r]);
        part[r] = fmaf(wq.y, rcp_sum_form(v.y, sv.y), part[r]);
        part[r] = fmaf(wq.z, rcp_sum_form(v.z, sv.z), part[r]);
        part[r] = fmaf(wq.w, rcp_sum_form(v.w, sv.w), part[r]);
      }
    }
#pragma unroll
    for (int r = 0; r < kRowR; ++r) {
      const float tot = wave_allsum(part[r]);
      if (lane == 0) sc[r * SP + n] = tot;
    }
  }
}

// ST = storage type of a, s, V, gr (r) and C (out): float, or bf16_t for TSG_BF16.  P, w, gbias are fp32.
template <bool GATE, typename ST>
__global__ __launch_bounds__(kRowThreads) void scdm_long_fwd_kernel(
    const ST* __restrict__ a, const ST* __restrict__ s, const float* __restrict__ w, const ST* __restrict__ V, ST* __restrict__ C,
    float* __restrict__ P, const ST* __restrict__ gr, const float* __restrict__ gbias, int B, int T, int N, int H, int Ds, int tiles) {
  constexpr int R = kRowR, TT = kRowTT;
  const int HP = roundup256(H), SP = roundup16(N), NPAD = (N + 3) & ~3;
  extern __shared__ __align__(16) float lds[];
  float* Es = lds;                       // [kNC][HP]
  float* Wl = Es + kNC * HP;             // [HP]   -2 w (0 beyond H)
  float* Sc = Wl + HP;                   // [TT][SP]  raw scores, then P (0 beyond N)
  int* Fl = reinterpret_cast<int*>(Sc + TT * SP);      // [kMaxChunks]  the chunk holds an s beyond the clamp

  const int tid = threadIdx.x, lane = tid & 63, wv = wave_id();
  const int bid = xcd_remap(blockIdx.x, gridDim.x, tiles);
  const int b = bid / tiles, t_tile = (bid % tiles) * TT;
  const ST* ab = a + (size_t)b * T * H;
  const ST* sb = s + (size_t)b * N * H;
  if (tid < kMaxChunks) Fl[tid] = 0;
  lds_barrier();

  typedef typename Raw4T<ST>::type Raw4;
  Raw4 q[R][4];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int t = t_tile + wv * R + r;
    const ST* row = ab + (size_t)(t < T ? t : T - 1) * H + lane * 4;
#pragma unroll
    for (int i = 0; i < 4; ++i) q[r][i] = (i * 256 + lane * 4 < H) ? ldraw4(row + i * 256) : zero_raw4(row);
  }
  bool abig = false;
#pragma unroll
  for (int r = 0; r < R; ++r)
#pragma unroll
    for (int i = 0; i < 4; ++i) abig = abig || beyond_clamp(cvt4(q[r][i]));
  const bool a_beyond = wave_any(abig);
  for (int k = tid * 4; k < HP; k += 4 * kRowThreads) {
    float4 wq = make_float4(0.f, 0.f, 0.f, 0.f);
    if (k < H) wq = *reinterpret_cast<const float4*>(w + k);
    *reinterpret_cast<float4*>(Wl + k) = make_float4(-2.f * wq.x, -2.f * wq.y, -2.f * wq.z, -2.f * wq.w);
  }

  // ---- phase 1: raw scores, one word chunk at a time ------------------------------------------------------------------------
  for (int c0 = 0; c0 < N; c0 += kNC) {
    if (c0) lds_barrier();                               // the previous chunk's readers are done
    stage_words<true>(Es, sb, c0, N, H, HP, tid, Fl + c0 / kNC);
    lds_barrier();
    const bool sum_form = a_beyond || __builtin_amdgcn_readfirstlane(Fl[c0 / kNC]) != 0;
    if (sum_form) {                                      // an operand beyond the clamp: out of line, so that the product form keeps its registers
      fwd_chunk_sum_form<ST>(ab, sb, Wl, Sc + wv * R * SP + c0, t_tile + wv * R, T, N, H, HP, SP, c0, lane);
      continue;
    }
    float acc[R][kNC];
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
      for (int n = 0; n < kNC; ++n) acc[r][n] = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (i * 256 < HP) {
        const int k = i * 256 + lane * 4;
        float Ea[R][4];
#pragma unroll
        for (int r = 0; r < R; ++r) {
          const float4 e = exp2x4(cvt4(q[r][i]));
          Ea[r][0] = e.x; Ea[r][1] = e.y; Ea[r][2] = e.z; Ea[r][3] = e.w;
        }
        const float4 wq = *reinterpret_cast<const float4*>(Wl + k);
        const float w2[4] = {wq.x, wq.y, wq.z, wq.w};
        long_score_step<R>(Ea, Es + k, HP, w2, acc);
      }
    }
#pragma unroll
    for (int r = 0; r < R; ++r) store_chunk_sums(acc[r], Sc + (wv * R + r) * SP + c0, lane);
  }
  lds_barrier();

  // ---- softmax over the N words of each row: lane l owns words l and l + 64 --------------------------------------------------
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int row = wv * R + r, t = t_tile + row;
    float* sr = Sc + row * SP;
    const bool v0 = lane < N, v1 = lane + 64 < N;
    const float e0 = v0 ? sr[lane] : -3.0e38f, e1 = v1 ? sr[lane + 64] : -3.0e38f;
    const float m = wave_allmax(fmaxf(e0, e1));
    float p0 = v0 ? fast_exp2((e0 - m) * kLog2e) : 0.f, p1 = v1 ? fast_exp2((e1 - m) * kLog2e) : 0.f;
    const float inv = 1.f / wave_allsum(p0 + p1);
    p0 *= inv; p1 *= inv;
    if (lane < SP) sr[lane] = p0;
    if (lane + 64 < SP) sr[lane + 64] = p1;
    if (t < T) {
      float* pr = P + ((size_t)b * T + t) * N;
      if (v0) pr[lane] = p0;
      if (v1) pr[lane + 64] = p1;
    }
  }
  lds_barrier();

  // ---- phase 2: C = P @ V, one column pair per thread, the tile's 32 rows in registers ------------------------------------
  const ST* Vb = V + (size_t)b * N * Ds;
  for (int j = tid * 2; j < Ds; j += 2 * kRowThreads) {
    float2 acc[TT];
#pragma unroll
    for (int i = 0; i < TT; ++i) acc[i] = make_float2(0.f, 0.f);
    typedef typename Raw2T<ST>::type Raw2;
    Raw2 cur[4], nxt[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) cur[u] = ldraw2(Vb + (size_t)(u < N ? u : N - 1) * Ds + j);
    for (int n4 = 0; n4 < NPAD; n4 += 4) {
#pragma unroll
      for (int u = 0; u < 4; ++u) {                      // the next four words' pieces fly during this group's FMAs
        const int n = n4 + 4 + u;
        nxt[u] = ldraw2(Vb + (size_t)(n < N ? n : N - 1) * Ds + j);      // (P is 0 beyond N: a repeated last row adds nothing)
      }
      float2 v[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) v[u] = cvt2(cur[u]);
#pragma unroll
      for (int i = 0; i < TT; ++i) {
        const float4 p = *reinterpret_cast<const float4*>(Sc + i * SP + n4);       // one address per wave: a broadcast read
        acc[i].x = fmaf(p.w, v[3].x, fmaf(p.z, v[2].x, fmaf(p.y, v[1].x, fmaf(p.x, v[0].x, acc[i].x))));
        acc[i].y = fmaf(p.w, v[3].y, fmaf(p.z, v[2].y, fmaf(p.y, v[1].y, fmaf(p.x, v[0].y, acc[i].y))));
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) cur[u] = nxt[u];
    }
    float2 gb = make_float2(0.f, 0.f);
    if (GATE) gb = *reinterpret_cast<const float2*>(gbias + j);
#pragma unroll
    for (int i = 0; i < TT; ++i) {
      const int t = t_tile + i;
      if (t < T) {
        const size_t off = ((size_t)b * T + t) * Ds + j;
        float2 o = acc[i];
        if (GATE) {
          const float2 rr = ld2(gr + off);
          o = make_float2(rr.x * sigmoidf(o.x + gb.x), rr.y * sigmoidf(o.y + gb.y));
        }
        st2(C + off, o);
      }
    }
  }
}

// ------------------------------------------------------------------------------------------
// backward
// ------------------------------------------------------------------------------------------
// rows: de (and, gate-fused, dr and dz) for the 32 rows of a tile.  dY = dC, or dout where GATE.
template <bool GATE, typename ST>
__global__ __launch_bounds__(kRowThreads) void scdm_long_bwd_rows_kernel(
    const ST* __restrict__ V, const float* __restrict__ P, const ST* __restrict__ dY, const ST* __restrict__ gr,
    const float* __restrict__ gbias, ST* __restrict__ dr, float* __restrict__ de, float* __restrict__ dG,
    int B, int T, int N, int Ds, int tiles) {
  constexpr int R = kRowR, TT = kRowTT;
  const int DP = roundup256(Ds), SP = roundup16(N), NPAD = (N + 3) & ~3;
  extern __shared__ __align__(16) float lds[];
  float* Vl = lds;                       // [kNC][DP]
  float* Pl = Vl + kNC * DP;             // [TT][SP]
  float* Dl = Pl + TT * SP;              // [TT][SP]  dP

  const int tid = threadIdx.x, lane = tid & 63, wv = wave_id();
  const int bid = xcd_remap(blockIdx.x, gridDim.x, tiles);
  const int b = bid / tiles, t_tile = (bid % tiles) * TT;
  const ST* Vb = V + (size_t)b * N * Ds;

  for (int idx = tid; idx < TT * SP; idx += kRowThreads) {
    const int row = idx / SP, n = idx % SP, t = t_tile + row;
    Pl[idx] = (t < T && n < N) ? P[((size_t)b * T + t) * N + n] : 0.f;
  }
  float4 g[R][4];                        // the wave's dY rows (zero for rows beyond T and columns beyond Ds); dz where GATE
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int t = t_tile + wv * R + r;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int col = i * 256 + lane * 4;
      g[r][i] = (t < T && col < Ds) ? ld4(dY + ((size_t)b * T + t) * Ds + col) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
  }

  if (GATE) {
    float4 z[R][4];
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
      for (int i = 0; i < 4; ++i) z[r][i] = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int c0 = 0; c0 < N; c0 += kNC) {
      if (c0) lds_barrier();
      stage_words<false>(Vl, Vb, c0, N, Ds, DP, tid);
      lds_barrier();
#pragma unroll 4
      for (int n = 0; n < kNC; ++n) {
        float p[R];
#pragma unroll
        for (int r = 0; r < R; ++r) p[r] = Pl[(wv * R + r) * SP + c0 + n];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          if (i * 256 < DP) {
            const float4 v = *reinterpret_cast<const float4*>(Vl + n * DP + i * 256 + lane * 4);
#pragma unroll
            for (int r = 0; r < R; ++r) {
              z[r][i].x = fmaf(p[r], v.x, z[r][i].x); z[r][i].y = fmaf(p[r], v.y, z[r][i].y);
              z[r][i].z = fmaf(p[r], v.z, z[r][i].z); z[r][i].w = fmaf(p[r], v.w, z[r][i].w);
            }
          }
        }
      }
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int t = t_tile + wv * R + r;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int col = i * 256 + lane * 4;
        if (t < T && col < Ds) {
          const size_t off = ((size_t)b * T + t) * Ds + col;
          const float4 gb = *reinterpret_cast<const float4*>(gbias + col);
          const float4 rr = ld4(gr + off);
          const float4 sg = make_float4(sigmoidf(z[r][i].x + gb.x), sigmoidf(z[r][i].y + gb.y), sigmoidf(z[r][i].z + gb.z), sigmoidf(z[r][i].w + gb.w));
          const float4 go = g[r][i];
          st4(dr + off, make_float4(go.x * sg.x, go.y * sg.y, go.z * sg.z, go.w * sg.w));
          const float4 dz = make_float4(go.x * rr.x * (sg.x - sg.x * sg.x), go.y * rr.y * (sg.y - sg.y * sg.y),
                                        go.z * rr.z * (sg.z - sg.z * sg.z), go.w * rr.w * (sg.w - sg.w * sg.w));
          *reinterpret_cast<float4*>(dG + off) = dz;
          g[r][i] = dz;
        }
      }
    }
    lds_barrier();                                       // every wave is done with the last V chunk of the z pass
  }

  // dP[t,n] = sum_j dz[t,j] V[n,j]
  for (int c0 = 0; c0 < N; c0 += kNC) {
    if (c0) lds_barrier();
    stage_words<false>(Vl, Vb, c0, N, Ds, DP, tid);
    lds_barrier();
    float acc[R][kNC];
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
      for (int n = 0; n < kNC; ++n) acc[r][n] = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (i * 256 < DP) {
#pragma unroll
        for (int n = 0; n < kNC; ++n) {
          const float4 v = *reinterpret_cast<const float4*>(Vl + n * DP + i * 256 + lane * 4);
#pragma unroll
          for (int r = 0; r < R; ++r)
            acc[r][n] = fmaf(g[r][i].w, v.w, fmaf(g[r][i].z, v.z, fmaf(g[r][i].y, v.y, fmaf(g[r][i].x, v.x, acc[r][n]))));
        }
      }
    }
#pragma unroll
    for (int r = 0; r < R; ++r) store_chunk_sums(acc[r], Dl + (wv * R + r) * SP + c0, lane);
  }
  lds_barrier();

  // de = P (dP - <P, dP>), zero in the row's padding
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int row = wv * R + r, t = t_tile + row;
    const bool v0 = lane < SP, v1 = lane + 64 < SP;
    const float p0 = v0 ? Pl[row * SP + lane] : 0.f, p1 = v1 ? Pl[row * SP + lane + 64] : 0.f;
    const float d0 = v0 ? Dl[row * SP + lane] : 0.f, d1 = v1 ? Dl[row * SP + lane + 64] : 0.f;
    const float dot = wave_allsum(fmaf(p0, d0, p1 * d1));
    if (t < T) {
      float* der = de + ((size_t)b * T + t) * NPAD;
      if (lane < NPAD) der[lane] = p0 * (d0 - dot);
      if (lane + 64 < NPAD) der[lane + 64] = p1 * (d1 - dot);
    }
  }
}

// da: the forward's tiling with de as the weights of q = r (1 - r).
template <typename ST>
__global__ __launch_bounds__(kRowThreads) void scdm_long_bwd_da_kernel(
    const ST* __restrict__ a, const ST* __restrict__ s, const float* __restrict__ w, const float* __restrict__ de, ST* __restrict__ da,
    int B, int T, int N, int H, int tiles) {
  constexpr int R = kDaR, TT = kDaTT;
  const int HP = roundup256(H), SP = roundup16(N), NPAD = (N + 3) & ~3;
  extern __shared__ __align__(16) float lds[];
  float* Es = lds;                       // [kNC][HP]
  float* Dl = Es + kNC * HP;             // [TT][SP]  de (0 beyond N and T)
  int* Fl = reinterpret_cast<int*>(Dl + TT * SP);      // [kMaxChunks]  the chunk holds an s beyond the clamp

  const int tid = threadIdx.x, lane = tid & 63, wv = wave_id();
  const int bid = xcd_remap(blockIdx.x, gridDim.x, tiles);
  const int b = bid / tiles, t_tile = (bid % tiles) * TT;
  const ST* ab = a + (size_t)b * T * H;
  const ST* sb = s + (size_t)b * N * H;
  if (tid < kMaxChunks) Fl[tid] = 0;
  lds_barrier();

  typedef typename Raw4T<ST>::type Raw4;
  Raw4 q[R][4];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int t = t_tile + wv * R + r;
    const ST* row = ab + (size_t)(t < T ? t : T - 1) * H + lane * 4;
#pragma unroll
    for (int i = 0; i < 4; ++i) q[r][i] = (i * 256 + lane * 4 < H) ? ldraw4(row + i * 256) : zero_raw4(row);
  }
  bool abig = false;
#pragma unroll
  for (int r = 0; r < R; ++r)
#pragma unroll
    for (int i = 0; i < 4; ++i) abig = abig || beyond_clamp(cvt4(q[r][i]));
  const bool a_beyond = wave_any(abig);
  for (int idx = tid; idx < TT * SP; idx += kRowThreads) {
    const int row = idx / SP, n = idx % SP, t = t_tile + row;
    Dl[idx] = (t < T && n < NPAD) ? de[((size_t)b * T + t) * NPAD + n] : 0.f;
  }
  float dacc[R][4][4];
#pragma unroll
  for (int r = 0; r < R; ++r)
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int c = 0; c < 4; ++c) dacc[r][i][c] = 0.f;

  for (int c0 = 0; c0 < N; c0 += kNC) {
    if (c0) lds_barrier();
    stage_words<true>(Es, sb, c0, N, H, HP, tid, Fl + c0 / kNC);
    lds_barrier();
    const bool sum_form = a_beyond || __builtin_amdgcn_readfirstlane(Fl[c0 / kNC]) != 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (i * 256 < HP) {
        const float* esp = Es + i * 256 + lane * 4;
        if (sum_form) {                                  // (see rcp_sum_form)
          const int k = i * 256 + lane * 4;
          float av[R][4];
#pragma unroll
          for (int r = 0; r < R; ++r) {
            const float4 v = cvt4(q[r][i]);
            av[r][0] = v.x; av[r][1] = v.y; av[r][2] = v.z; av[r][3] = v.w;
          }
#pragma unroll 4
          for (int n = 0; n < kNC; ++n) {
            const float4 sv = (k < H && c0 + n < N) ? ld4(sb + (size_t)(c0 + n) * H + k) : make_float4(0.f, 0.f, 0.f, 0.f);
            const float s4[4] = {sv.x, sv.y, sv.z, sv.w};
#pragma unroll
            for (int r = 0; r < R; ++r) {
              const float d = Dl[(wv * R + r) * SP + c0 + n];
#pragma unroll
              for (int c = 0; c < 4; ++c) {
                const float rr = rcp_sum_form(av[r][c], s4[c]);
                dacc[r][i][c] = fmaf(d, fmaf(-rr, rr, rr), dacc[r][i][c]);
              }
            }
          }
          continue;
        }
        float Ea[R][4];
#pragma unroll
        for (int r = 0; r < R; ++r) {
          const float4 e = exp2x4(cvt4(q[r][i]));
          Ea[r][0] = e.x; Ea[r][1] = e.y; Ea[r][2] = e.z; Ea[r][3] = e.w;
        }
#pragma unroll
        for (int n4 = 0; n4 < kNC; n4 += 4) {
          float d[R][4];
#pragma unroll
          for (int r = 0; r < R; ++r) {
            const float4 d4 = *reinterpret_cast<const float4*>(Dl + (wv * R + r) * SP + c0 + n4);
            d[r][0] = d4.x; d[r][1] = d4.y; d[r][2] = d4.z; d[r][3] = d4.w;
          }
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            const float4 ev = *reinterpret_cast<const float4*>(esp + (n4 + u) * HP);
            const float e4[4] = {ev.x, ev.y, ev.z, ev.w};
#pragma unroll
            for (int r = 0; r < R; ++r)
#pragma unroll
              for (int c = 0; c < 4; ++c) {
                const float rr = fast_rcp(fmaf(Ea[r][c], e4[c], 1.f));
                dacc[r][i][c] = fmaf(d[r][u], fmaf(-rr, rr, rr), dacc[r][i][c]);
              }
          }
          __builtin_amdgcn_sched_barrier(0);
        }
      }
    }
  }
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int t = t_tile + wv * R + r;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int k = i * 256 + lane * 4;
      if (t < T && k < H) {
        const float4 wq = *reinterpret_cast<const float4*>(w + k);
        st4(da + ((size_t)b * T + t) * H + k, make_float4(4.f * wq.x * dacc[r][i][0], 4.f * wq.y * dacc[r][i][1],
                                                           4.f * wq.z * dacc[r][i][2], 4.f * wq.w * dacc[r][i][3]));
      }
    }
  }
}

// Epilogue of the column-sliced kernels: the 4 waves' partial [kNC][256] tiles are summed through LDS (8 words at a time) and
// out[n][col .. col+3] = scale[col ..] * sum is stored once.  `scale` may be nullptr (= 1).
template <typename ST>
__device__ __forceinline__ void cols_reduce_store(const float4 (&acc)[kNC], float* red /* [kColWaves][8][256] */, ST* __restrict__ outb,
                                                  const float* __restrict__ scale, float mul, int c0, int N, int col0, int W, int tid) {
  const int lane = tid & 63, wv = tid >> 6;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    __syncthreads();
#pragma unroll
    for (int u = 0; u < 8; ++u) *reinterpret_cast<float4*>(red + ((wv * 8 + u) * 256) + lane * 4) = acc[h * 8 + u];
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int idx = tid + i * kColThreads, nl = idx >> 6, qd = idx & 63;
      float4 sum = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
      for (int x = 0; x < kColWaves; ++x) {
        const float4 v = *reinterpret_cast<const float4*>(red + ((x * 8 + nl) * 256) + qd * 4);
        sum.x += v.x; sum.y += v.y; sum.z += v.z; sum.w += v.w;
      }
      const int n = c0 + h * 8 + nl, col = col0 + qd * 4;
      if (n < N && col < W) {
        float4 sc = make_float4(mul, mul, mul, mul);
        if (scale) {
          const float4 wq = *reinterpret_cast<const float4*>(scale + col);
          sc = make_float4(mul * wq.x, mul * wq.y, mul * wq.z, mul * wq.w);
        }
        st4(outb + (size_t)n * W + col, make_float4(sc.x * sum.x, sc.y * sum.y, sc.z * sum.z, sc.w * sum.w));
      }
    }
  }
}
// ... and of a per-column sum: dst[col] += mul * (sum over the waves), one atomic per column and workgroup
__device__ __forceinline__ void cols_reduce_atomic(float4 v, float* red, float* __restrict__ dst, float mul, int col0, int W, int tid) {
  const int lane = tid & 63, wv = tid >> 6;
  __syncthreads();
  *reinterpret_cast<float4*>(red + wv * 256 + lane * 4) = v;
  __syncthreads();
  float sum = 0.f;
#pragma unroll
  for (int x = 0; x < kColWaves; ++x) sum += red[x * 256 + tid];
  if (col0 + tid < W) atomicAdd(dst + col0 + tid, mul * sum);
}

// ds and dw: workgroup = (b, 256-column slice, 16-word chunk); the chunk's Es quads live in registers, the 4 waves share the T rows.
// Two instantiations are launched one after the other and every workgroup belongs to exactly one: it first looks through its s quads and its
// a rows for an operand beyond the clamp (see rcp_sum_form); SUM = false goes on only where there is none (the product form, Es = exp(2s) in
// registers), SUM = true only where there is one (the sum form, s itself in registers).  One more read of the a slice from L2 each; the
// product form keeps its registers, and each output is still written by one workgroup.
template <typename ST, bool SUM>
__global__ __launch_bounds__(kColThreads) void scdm_long_bwd_ds_kernel(
    const ST* __restrict__ a, const ST* __restrict__ s, const float* __restrict__ w, const float* __restrict__ de, ST* __restrict__ ds,
    float* __restrict__ dw, int T, int N, int H, int slices) {
  __shared__ __align__(16) float red[kColWaves * 8 * 256];
  __shared__ int beyond;
  const int tid = threadIdx.x, lane = tid & 63, wv = wave_id();
  const int b = blockIdx.x, slice = blockIdx.y % slices, c0 = (blockIdx.y / slices) * kNC;
  const int NPAD = (N + 3) & ~3;
  const int col0 = slice * 256, k = col0 + lane * 4;
  const bool kok = k < H;
  typedef typename Raw4T<ST>::type Raw4;
  const ST* ab = a + (size_t)b * T * H + (kok ? k : 0);

  if (tid == 0) beyond = 0;
  __syncthreads();
  float4 es[kNC], acc[kNC];                             // es: exp(2 s), or s itself where SUM
  bool big = false;
#pragma unroll
  for (int u = 0; u < kNC; ++u) {
    const int n = c0 + u;
    const float4 sv = (kok && n < N) ? ld4(s + ((size_t)b * N + n) * H + k) : make_float4(0.f, 0.f, 0.f, 0.f);
    big = big || beyond_clamp(sv);
    es[u] = SUM ? sv : ((kok && n < N) ? exp2x4(sv) : make_float4(0.f, 0.f, 0.f, 0.f));
    acc[u] = make_float4(0.f, 0.f, 0.f, 0.f);
  }
  for (int t = wv; t < T; t += 4 * kColWaves) {         // four rows in flight
    Raw4 v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int tj = t + j * kColWaves;
      v[j] = ldraw4(ab + (size_t)(tj < T ? tj : T - 1) * H);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) big = big || (kok && beyond_clamp(cvt4(v[j])));
  }
  if (wave_any(big) && lane == 0) beyond = 1;
  __syncthreads();
  if ((beyond != 0) != SUM) return;                     // the other instantiation's workgroup

  float4 dwacc = make_float4(0.f, 0.f, 0.f, 0.f);
  Raw4 nxt = ldraw4(ab + (size_t)(wv < T ? wv : T - 1) * H);
  for (int t = wv; t < T; t += kColWaves) {
    const Raw4 cur = nxt;
    const int tn = t + kColWaves;
    nxt = ldraw4(ab + (size_t)(tn < T ? tn : T - 1) * H);          // the next row flies during this row's 64 reciprocals
    const float4 araw = cvt4(cur);
    const float4 e = SUM ? araw : exp2x4(araw);
    const float Ea[4] = {e.x, e.y, e.z, e.w};
    const float* der = de + ((size_t)b * T + t) * NPAD + c0;         // wave-uniform
#pragma unroll
    for (int u = 0; u < kNC; ++u) {
      const float d = (c0 + u < NPAD) ? der[u] : 0.f;
      const float e4[4] = {es[u].x, es[u].y, es[u].z, es[u].w};
      float qv[4], rr[4];
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        rr[c] = SUM ? rcp_sum_form(Ea[c], e4[c]) : fast_rcp(fmaf(Ea[c], e4[c], 1.f));
        qv[c] = fmaf(-rr[c], rr[c], rr[c]);
      }
      acc[u].x = fmaf(d, qv[0], acc[u].x); acc[u].y = fmaf(d, qv[1], acc[u].y);
      acc[u].z = fmaf(d, qv[2], acc[u].z); acc[u].w = fmaf(d, qv[3], acc[u].w);
      dwacc.x = fmaf(d, rr[0], dwacc.x); dwacc.y = fmaf(d, rr[1], dwacc.y);
      dwacc.z = fmaf(d, rr[2], dwacc.z); dwacc.w = fmaf(d, rr[3], dwacc.w);
    }
  }
  cols_reduce_store<ST>(acc, red, ds + (size_t)b * N * H, w, 4.f, c0, N, col0, H, tid);
  cols_reduce_atomic(dwacc, red, dw, -2.f, col0, H, tid);
}

// dV (dsent / dVW) and dgbias: the same slicing; dz = dC (storage type) or, gate-fused, the fp32 rows the rows kernel left.
template <bool GATE, typename ST>
__global__ __launch_bounds__(kColThreads) void scdm_long_bwd_dv_kernel(
    const float* __restrict__ P, const void* __restrict__ dz_, ST* __restrict__ dV, float* __restrict__ dgbias,
    int T, int N, int Ds, int slices) {
  typedef typename std::conditional<GATE, float, ST>::type ZT;
  const ZT* dz = static_cast<const ZT*>(dz_);
  __shared__ __align__(16) float red[kColWaves * 8 * 256];
  const int tid = threadIdx.x, lane = tid & 63, wv = wave_id();
  const int b = blockIdx.x, slice = blockIdx.y % slices, c0 = (blockIdx.y / slices) * kNC;
  const int col0 = slice * 256, col = col0 + lane * 4;
  const bool cok = col < Ds;

  float4 acc[kNC];
#pragma unroll
  for (int u = 0; u < kNC; ++u) acc[u] = make_float4(0.f, 0.f, 0.f, 0.f);
  float4 bsum = make_float4(0.f, 0.f, 0.f, 0.f);
  typedef typename Raw4T<ZT>::type Raw4;
  const ZT* zb = dz + (size_t)b * T * Ds + (cok ? col : 0);
  Raw4 nxt = ldraw4(zb + (size_t)(wv < T ? wv : T - 1) * Ds);
  for (int t = wv; t < T; t += kColWaves) {
    const Raw4 cur = nxt;
    const int tn = t + kColWaves;
    nxt = ldraw4(zb + (size_t)(tn < T ? tn : T - 1) * Ds);
    const float4 z = cvt4(cur);
    const float* pr = P + ((size_t)b * T + t) * N + c0;               // wave-uniform
#pragma unroll
    for (int u = 0; u < kNC; ++u) {
      const float p = (c0 + u < N) ? pr[u] : 0.f;
      acc[u].x = fmaf(p, z.x, acc[u].x); acc[u].y = fmaf(p, z.y, acc[u].y);
      acc[u].z = fmaf(p, z.z, acc[u].z); acc[u].w = fmaf(p, z.w, acc[u].w);
    }
    bsum.x += z.x; bsum.y += z.y; bsum.z += z.z; bsum.w += z.w;
  }
  cols_reduce_store<ST>(acc, red, dV + (size_t)b * N * Ds, nullptr, 1.f, c0, N, col0, Ds, tid);
  if (GATE && c0 == 0) cols_reduce_atomic(bsum, red, dgbias, 1.f, col0, Ds, tid);
}

// ------------------------------------------------------------------------------------------
// host
// ------------------------------------------------------------------------------------------
int check_long(const char* fn, std::initializer_list<const void*> ptrs, int B, int T, int N, int H, int Ds, int dtype) {
  if (int rc = check_scdm_args(fn, ptrs, B, T, N, kLongMaxWords, H, Ds, dtype)) return rc;
  if (H > kLongMaxH) return set_error(TSG_E_SHAPE, "%s: H=%d > %d not supported", fn, H, kLongMaxH);
  if (Ds > kLongMaxDs) return set_error(TSG_E_SHAPE, "%s: Ds=%d > %d not supported", fn, Ds, kLongMaxDs);
  return 0;
}

long long long_ws_bytes(int B, int T, int N, int Ds, bool gate) {
  const long long rows = (long long)B * T;
  return 4LL * rows * roundup(N, 4) + (gate ? 4LL * rows * Ds : 0LL);      // de [B*T][roundup(N,4)], then dz [B*T][Ds]
}

template <bool GATE, typename ST>
int launch_long_fwd(const void* a, const void* s, const void* w, const void* V, void* C, void* P, const void* gr, const void* gbias,
                    int B, int T, int N, int H, int Ds, hipStream_t st) {
  const int tiles = cdiv(T, kRowTT);
  const size_t lds = sizeof(float) * ((size_t)(kNC + 1) * roundup256(H) + (size_t)kRowTT * roundup16(N) + kMaxChunks);
  auto kern = scdm_long_fwd_kernel<GATE, ST>;
  if (hipError_t e = allow_lds(kern, lds)) return (int)e;
  hipLaunchKernelGGL(kern, dim3((unsigned)(B * tiles)), dim3(kRowThreads), lds, st, (const ST*)a, (const ST*)s, (const float*)w,
                     (const ST*)V, (ST*)C, (float*)P, (const ST*)gr, (const float*)gbias, B, T, N, H, Ds, tiles);
  return check_launch(GATE ? "scdm_long_gate_fwd" : "scdm_long_fwd");
}

template <bool GATE, typename ST>
int launch_long_bwd(const char* fn, const void* a, const void* s, const void* w, const void* V, const void* gbias, const void* gr,
                    const void* P, const void* dY, void* da, void* ds, void* dw, void* dV, void* dgbias, void* dr, void* ws,
                    long long ws_bytes, int B, int T, int N, int H, int Ds, hipStream_t st) {
  const long long need = long_ws_bytes(B, T, N, Ds, GATE);
  if (ws_bytes < need) return set_error(TSG_E_SHAPE, "%s: workspace of %lld B < %lld B (tsg_scdm_long_ws_bytes)", fn, ws_bytes, need);
  float* de = static_cast<float*>(ws);
  float* dG = GATE ? de + (size_t)B * T * roundup(N, 4) : nullptr;
  const int tiles = cdiv(T, kRowTT), chunks = cdiv(N, kNC);
  if (hipError_t e = zero3_async(dw, sizeof(float) * H, GATE ? dgbias : nullptr, sizeof(float) * Ds, nullptr, 0, st)) return (int)e;
  {
    const size_t lds = sizeof(float) * ((size_t)kNC * roundup256(Ds) + 2 * (size_t)kRowTT * roundup16(N));
    auto kern = scdm_long_bwd_rows_kernel<GATE, ST>;
    if (hipError_t e = allow_lds(kern, lds)) return (int)e;
    hipLaunchKernelGGL(kern, dim3((unsigned)(B * tiles)), dim3(kRowThreads), lds, st, (const ST*)V, (const float*)P, (const ST*)dY,
                       (const ST*)gr, (const float*)gbias, (ST*)dr, de, dG, B, T, N, Ds, tiles);
    if (int rc = check_launch("scdm_long_bwd_rows")) return rc;
  }
  {
    const int da_tiles = cdiv(T, kDaTT);
    const size_t lds = sizeof(float) * ((size_t)kNC * roundup256(H) + (size_t)kDaTT * roundup16(N) + kMaxChunks);
    auto kern = scdm_long_bwd_da_kernel<ST>;
    if (hipError_t e = allow_lds(kern, lds)) return (int)e;
    hipLaunchKernelGGL(kern, dim3((unsigned)(B * da_tiles)), dim3(kRowThreads), lds, st, (const ST*)a, (const ST*)s, (const float*)w,
                       (const float*)de, (ST*)da, B, T, N, H, da_tiles);
    if (int rc = check_launch("scdm_long_bwd_da")) return rc;
  }
  {
    const int slices = cdiv(H, 256);
    hipLaunchKernelGGL((scdm_long_bwd_ds_kernel<ST, false>), dim3((unsigned)B, (unsigned)(slices * chunks)), dim3(kColThreads), 0, st,
                       (const ST*)a, (const ST*)s, (const float*)w, (const float*)de, (ST*)ds, (float*)dw, T, N, H, slices);
    if (int rc = check_launch("scdm_long_bwd_ds")) return rc;
    hipLaunchKernelGGL((scdm_long_bwd_ds_kernel<ST, true>), dim3((unsigned)B, (unsigned)(slices * chunks)), dim3(kColThreads), 0, st,
                       (const ST*)a, (const ST*)s, (const float*)w, (const float*)de, (ST*)ds, (float*)dw, T, N, H, slices);
    if (int rc = check_launch("scdm_long_bwd_ds (sum form)")) return rc;
  }
  {
    const int slices = cdiv(Ds, 256);
    hipLaunchKernelGGL((scdm_long_bwd_dv_kernel<GATE, ST>), dim3((unsigned)B, (unsigned)(slices * chunks)), dim3(kColThreads), 0, st,
                       (const float*)P, GATE ? (const void*)dG : dY, (ST*)dV, (float*)dgbias, T, N, Ds, slices);
    if (int rc = check_launch("scdm_long_bwd_dv")) return rc;
  }
  return 0;
}

}  // namespace
}  // namespace tsg

using namespace tsg;

extern "C" int tsg_scdm_long_max_words(void) { return kLongMaxWords; }

extern "C" long long tsg_scdm_long_ws_bytes(int B, int T, int N, int H, int Ds, int gate) {
  if (B <= 0 || T <= 0 || N <= 0 || N > kLongMaxWords || H <= 0 || Ds <= 0 || H % 4 || Ds % 4 || H > kLongMaxH || Ds > kLongMaxDs ||
      (long long)B * T >= (1LL << 31))
    return 0;                                            // (shapes the entry points reject)
  return long_ws_bytes(B, T, N, Ds, gate != 0);
}

extern "C" int tsg_scdm_long_fwd(const void* a, const void* s, const void* w, const void* sent, void* C, void* P,
                                 int B, int T, int N, int H, int Ds, int dtype, void* stream) {
  if (int rc = check_long("tsg_scdm_long_fwd", {a, s, w, sent, C, P}, B, T, N, H, Ds, dtype)) return rc;
  auto st = static_cast<hipStream_t>(stream);
  if (dtype == TSG_BF16) return launch_long_fwd<false, bf16_t>(a, s, w, sent, C, P, nullptr, nullptr, B, T, N, H, Ds, st);
  return launch_long_fwd<false, float>(a, s, w, sent, C, P, nullptr, nullptr, B, T, N, H, Ds, st);
}

extern "C" int tsg_scdm_long_gate_fwd(const void* a, const void* s, const void* w, const void* VW, const void* gbias, const void* r,
                                      void* out, void* P, int B, int T, int N, int H, int Ds, int dtype, void* stream) {
  if (int rc = check_long("tsg_scdm_long_gate_fwd", {a, s, w, VW, gbias, r, out, P}, B, T, N, H, Ds, dtype)) return rc;
  auto st = static_cast<hipStream_t>(stream);
  if (dtype == TSG_BF16) return launch_long_fwd<true, bf16_t>(a, s, w, VW, out, P, r, gbias, B, T, N, H, Ds, st);
  return launch_long_fwd<true, float>(a, s, w, VW, out, P, r, gbias, B, T, N, H, Ds, st);
}

extern "C" int tsg_scdm_long_bwd(const void* a, const void* s, const void* w, const void* sent, const void* P, const void* dC,
                                 void* da, void* ds, void* dw, void* dsent, void* ws, long long ws_bytes,
                                 int B, int T, int N, int H, int Ds, int dtype, void* stream) {
  const char* fn = "tsg_scdm_long_bwd";
  if (int rc = check_long(fn, {a, s, w, sent, P, dC, da, ds, dw, dsent, ws}, B, T, N, H, Ds, dtype)) return rc;
  auto st = static_cast<hipStream_t>(stream);
  if (dtype == TSG_BF16)
    return launch_long_bwd<false, bf16_t>(fn, a, s, w, sent, nullptr, nullptr, P, dC, da, ds, dw, dsent, nullptr, nullptr, ws, ws_bytes,
                                          B, T, N, H, Ds, st);
  return launch_long_bwd<false, float>(fn, a, s, w, sent, nullptr, nullptr, P, dC, da, ds, dw, dsent, nullptr, nullptr, ws, ws_bytes,
                                       B, T, N, H, Ds, st);
}

extern "C" int tsg_scdm_long_gate_bwd(const void* a, const void* s, const void* w, const void* VW, const void* gbias, const void* r,
                                      const void* P, const void* dout, void* da, void* ds, void* dw, void* dVW, void* dgbias, void* dr,
                                      void* ws, long long ws_bytes, int B, int T, int N, int H, int Ds, int dtype, void* stream) {
  const char* fn = "tsg_scdm_long_gate_bwd";
  if (int rc = check_long(fn, {a, s, w, VW, gbias, r, P, dout, da, ds, dw, dVW, dgbias, dr, ws}, B, T, N, H, Ds, dtype)) return rc;
  auto st = static_cast<hipStream_t>(stream);
  if (dtype == TSG_BF16)
    return launch_long_bwd<true, bf16_t>(fn, a, s, w, VW, gbias, r, P, dout, da, ds, dw, dVW, dgbias, dr, ws, ws_bytes, B, T, N, H, Ds, st);
  return launch_long_bwd<true, float>(fn, a, s, w, VW, gbias, r, P, dout, da, ds, dw, dVW, dgbias, dr, ws, ws_bytes, B, T, N, H, Ds, st);
}
