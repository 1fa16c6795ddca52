// Device-side input pipeline and span decoding of the grounding path for gfx950.
//
// The reference builds every batch on the host with numpy, one sample at a time, in 8 DataLoader workers feeding ONE GPU
// (grounding/dataset/charades.py, charades_pair_aug.py, data_augment.py); eight ranks on one host would contend for that.
// Here the per-batch work runs on the GPU that consumes it:
//   tsg_sample_clips      raw clip features -> the [T, D] rows the model reads, the six samplers of the reference's Charades
//                         and ActivityNet datasets (dataset/charades.py:177-269, dataset/anet.py:173-277) as one kernel body
//   tsg_pool_clips        its PAIR mode: adjacent-pair mean pooling of the raw i3d clips + zero pad + nfeats + frame stamps
//                         (CharadesDataSentence.generate_video_fts_data, dataset/charades.py:177-196)
//   tsg_sequence_masks    video / temporal / fore / back masks from (nfeats, span)
//                         (Sequence_mask, charades.py:12-18, as combined at charades.py:167-170 / charades_pair_aug.py:96-107)
//   tsg_moment_translate  the shuffling augmentation as an index gather (DataAugmentForTSG.gt_moment_translate,
//                         dataset/data_augment.py:135-156), insert position given or drawn from a counter-based hash
//   tsg_span_pred         argmax_{i,j} of the zero-filled upper-triangular start_i + end_j matrix, first maximum wins
//                         (span_pred, grounding/loss.py:53-70)
// All of it is integer / byte work bound by HBM (the gather and the pooling move B*T*D*4 bytes each way) or by latency
// (masks, decode).  Index outputs are bit-exact with the reference; feature outputs are copies / one rounded fp32 mean.
#include "tsg_common.h"

namespace tsg {
namespace {

constexpr int kThreads = 256;
constexpr int kRowsPerWg = 8;                 // feature rows per workgroup: 8 x D floats, all loads issued before the stores
constexpr int kUnroll = 8;                    // 16-byte vectors per thread in flight (tsg_sample_clips)
constexpr int kMaxSampleT = 16384;            // longest T tsg_sample_clips takes

__device__ __forceinline__ unsigned long long splitmix64(unsigned long long x) {
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}

// insert position of the shuffling augmentation when the caller does not provide one: uniform over [0, wo_len]
// (random.randint(0, wo_len), data_augment.py:149) from a counter-based hash of (seed, sample index): seedable, order-free
__device__ __forceinline__ int draw_cropin(unsigned long long seed, int b, int wo_len) {
  const unsigned long long h = splitmix64(seed ^ (0xD1B54A32D192ED03ull * (unsigned long long)(b + 1)));
  return (int)(((h >> 32) * (unsigned long long)(wo_len + 1)) >> 32);
}

struct Translate { int s, n, c, nf; bool noop; };

__device__ __forceinline__ Translate translate_of(const int* __restrict__ spans, const int* __restrict__ nfeats,
                                                  const int* __restrict__ cropin, unsigned long long seed, int b) {
  Translate tr;
  const int s = spans[2 * b], e = spans[2 * b + 1];
  tr.s = s; tr.n = e - s + 1; tr.nf = nfeats[b];
  tr.noop = tr.n <= 1 || tr.n >= tr.nf;                       // data_augment.py:138-139
  // a caller's insert position is clamped to the reference's range [0, nf - n], as tsg_moment_augment clamps its plan
  tr.c = tr.noop ? s : (cropin ? min(max(cropin[b], 0), tr.nf - tr.n) : draw_cropin(seed, b, tr.nf - tr.n));
  return tr;
}

// source row of output row t (-1 = zero row): [0,c) gap-closed rows, [c,c+n) the moment, then the rest of the gap-closed rows.
// The gap-closed sequence is rows [0, s) then rows [e+1, nf) at [s, nf-n), zeros after (data_augment.py:142-146); a moment that
// ends at or past nf (LG's end label T-1) leaves just rows [0, s) -- the output then holds e+1 > nf rows, as the reference's does.
__device__ __forceinline__ int translate_src(const Translate& tr, int t) {
  if (tr.noop) return t;
  if (t >= tr.c && t < tr.c + tr.n) return tr.s + (t - tr.c);
  const int i = t < tr.c ? t : t - tr.n;                      // index in the sequence without the moment
  if (i < tr.s) return i;
  return i < tr.nf - tr.n ? i + tr.n : -1;
}

__global__ __launch_bounds__(kThreads) void moment_translate_kernel(
    const float* __restrict__ video, const int* __restrict__ spans, const int* __restrict__ nfeats,
    const int* __restrict__ cropin, unsigned long long seed, float* __restrict__ out, int* __restrict__ new_spans,
    int B, int T, int D, int tiles) {
  const int b = blockIdx.x / tiles, t0 = (blockIdx.x % tiles) * kRowsPerWg;
  const Translate tr = translate_of(spans, nfeats, cropin, seed, b);
  if (blockIdx.x % tiles == 0 && threadIdx.x == 0) {
    new_spans[2 * b] = tr.c;                                  // no-op: the span itself (c = s, n = e - s + 1)
    new_spans[2 * b + 1] = tr.c + tr.n - 1;
  }
  const int d4 = D / 4, per_wg = kRowsPerWg * d4;
  const float4* vb = reinterpret_cast<const float4*>(video) + (size_t)b * T * d4;
  float4* ob = reinterpret_cast<float4*>(out) + (size_t)b * T * d4;
  for (int base = threadIdx.x; base < per_wg; base += 8 * kThreads) {
    float4 v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int idx = base + u * kThreads, r = idx / d4, k = idx % d4, t = t0 + r;
      v[u] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (idx < per_wg && t < T) {
        const int src = translate_src(tr, t);
        if (src >= 0 && src < T) v[u] = vb[(size_t)src * d4 + k];
      }
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int idx = base + u * kThreads, r = idx / d4, k = idx % d4, t = t0 + r;
      if (idx < per_wg && t < T) ob[(size_t)t * d4 + k] = v[u];
    }
  }
}

// ---- tsg_sample_clips: raw clip features -> [T, D] rows, one body for the reference's six samplers --------------------------
// Output row t of sample b is the mean of the raw rows [lo, lo + cnt) of that sample (cnt 1: a copy, cnt 0: a zero row); the mode
// only decides the windows and the labels.  Means are the reference's np.mean over float32 rows: a sequential fp32 sum in row
// order, then ONE correctly rounded fp32 division by the count.  The index arithmetic below is done in double exactly as the
// reference's Python / numpy forms it; contraction is off there (the build uses -ffp-contract=fast), because a fused
// start + i*delta or i*rate + 0.5 rounds differently from numpy in rare cases and moves a row.
struct Sampler {
  int mode, n, rows, nf;                      // raw clips, rows [0, rows) carry a window, the nfeats written out
  double rate;                                // F2S / F2S_114: n / duration
  double a0, a1, delta;                       // LG: np.arange(spos, n - 0.5, stride) = a0, a1, a0 + i*delta (i >= 2)
  int spos;
};

__device__ __forceinline__ unsigned long long spos_hash(unsigned long long seed, int b) {
  return splitmix64(seed ^ (0xD1B54A32D192ED03ull * (unsigned long long)(b + 1)) ^ 0x8CB92BA72F3D8DD7ull);
}

// LG's training draw: np.random.random_integers(0, random_end) with random_end = stride - 0.5, minus 1 when integral; it draws
// from [0, int(random_end)] INCLUSIVE (charades.py:209-215, anet.py:243-249)
__device__ __forceinline__ int lg_spos_hi(double stride) {
#pragma clang fp contract(off)
  double re = stride - 0.5;
  if (re == floor(re)) re = re - 1.0;
  return (int)re;
}

__device__ __forceinline__ Sampler sampler_of(int mode, int n, int T, const double* __restrict__ durations, int train,
                                              unsigned long long seed, const int* __restrict__ spos_in, int b) {
#pragma clang fp contract(off)
  Sampler sp{mode, n, 0, 0, 0.0, 0.0, 0.0, 0.0, 0};
  switch (mode) {
    case TSG_SAMPLE_PAIR: sp.rows = sp.nf = min((n + 1) / 2, T); break;        // charades.py:185-193
    case TSG_SAMPLE_TRIPLE: sp.rows = sp.nf = min((n + 2) / 3, T); break;      // charades.py:255-267
    case TSG_SAMPLE_ONE_TO_ONE: sp.rows = sp.nf = min(n, T); break;            // anet.py:201-205
    case TSG_SAMPLE_F2S:
    case TSG_SAMPLE_F2S_114: {                                // rows i < duration (and < T): anet.py:185-186, :221-222
      const double dur = durations[b];
      const int cnt = dur > 0.0 ? (dur >= (double)T ? T : (int)ceil(dur)) : 0;
      sp.rate = (double)n / dur;
      sp.rows = n > 0 ? cnt : 0;                              // no clips: the reference raises; zero rows here
      sp.nf = mode == TSG_SAMPLE_F2S ? cnt : n;               // 114 returns the clip count itself, NOT clamped to T (anet.py:230)
      break;
    }
    default: {                                                // TSG_SAMPLE_LG (charades.py:198-243, anet.py:232-277)
      const double stride = n <= T ? 1.0 : (double)n / (double)T;
      if (spos_in) sp.spos = spos_in[b];
      else if (train) {
        const int hi = lg_spos_hi(stride);
        sp.spos = hi <= 0 ? 0 : (int)(((spos_hash(seed, b) >> 32) * (unsigned long long)(hi + 1)) >> 32);
      }
      sp.a0 = (double)sp.spos;
      sp.a1 = sp.a0 + stride;                                 // numpy's arange: second element start + step,
      sp.delta = sp.a1 - sp.a0;                               // then start + i * ((start + step) - start)
      sp.rows = sp.nf = min(n, T);
    }
  }
  return sp;
}

// LG: the arange element i, rounded half to even (np.round)
__device__ __forceinline__ double lg_pos(const Sampler& sp, int i) {
#pragma clang fp contract(off)
  const double v = i == 0 ? sp.a0 : (i == 1 ? sp.a1 : sp.a0 + (double)i * sp.delta);
  return rint(v);
}

// window [lo, lo + cnt) of output row t (cnt 0: zero row); every lo is clamped into the sample's rows
__device__ __forceinline__ int2 window_of(const Sampler& sp, int t) {
#pragma clang fp contract(off)
  const int n = sp.n;
  if (t >= sp.rows || n <= 0) return make_int2(0, 0);
  switch (sp.mode) {
    case TSG_SAMPLE_PAIR: return make_int2(2 * t, min(2, n - 2 * t));
    case TSG_SAMPLE_TRIPLE: return make_int2(3 * t, min(3, n - 3 * t));
    case TSG_SAMPLE_ONE_TO_ONE: return make_int2(t, 1);
    case TSG_SAMPLE_F2S: {                                    // max(0, floor(i * rate)) (anet.py:187)
      const double f = floor((double)t * sp.rate);
      return make_int2(f >= (double)(n - 1) ? n - 1 : (int)f, 1);
    }
    case TSG_SAMPLE_F2S_114: {                                // anet.py:223-228
      const double fs = (double)t * sp.rate + 0.5, fe = (double)(t + 1) * sp.rate + 0.5;
      const int st = fs >= (double)(n - 1) ? n - 1 : (int)fs;
      const int en = fe >= (double)(n + 1) ? n + 1 : (int)fe;     // int(fe) > n, without converting a huge fe
      return (en > n || en <= st) ? make_int2(st, 1) : make_int2(st, en - st);
    }
    default: {                                                // LG: feat[s[t]]
      const double v = lg_pos(sp, t);
      return make_int2(v >= (double)(n - 1) ? n - 1 : (v <= 0.0 ? 0 : (int)v), 1);
    }
  }
}

template <typename ST>
__global__ __launch_bounds__(kThreads) void sample_clips_kernel(
    const float* __restrict__ raw, const long long* __restrict__ offsets, const double* __restrict__ timestamps,
    const double* __restrict__ durations, int mode, int train, unsigned long long seed, const int* __restrict__ spos_in,
    ST* __restrict__ out, int* __restrict__ nfeats, int* __restrict__ framestps, int* __restrict__ spos_out, int T, int D,
    int tiles) {
  __shared__ int2 win[kRowsPerWg];
  __shared__ int label[2];
  const int b = blockIdx.x / tiles, tile = blockIdx.x % tiles, t0 = tile * kRowsPerWg;
  const long long r0 = offsets[b];
  const int n = (int)(offsets[b + 1] - r0);
  const Sampler sp = sampler_of(mode, n, T, durations, train, seed, spos_in, b);
  if (threadIdx.x < kRowsPerWg) win[threadIdx.x] = window_of(sp, t0 + threadIdx.x);
  if (tile == 0) {                                            // the sample's labels (workgroup-uniform branch)
    if (mode == TSG_SAMPLE_LG) {
      // s[i] <= pos < s[i+1] over i < len(s) - 1, the last match wins; defaults 0 and T - 1 (charades.py:217-237)
#pragma clang fp contract(off)
      if (threadIdx.x < 2) label[threadIdx.x] = -1;
      __syncthreads();
      const double dur = durations[b];
      const double ps = (double)(n - 1) * fmin(fmax(timestamps[2 * b] / dur, 0.0), 1.0);
      const double pe = (double)(n - 1) * fmin(fmax(timestamps[2 * b + 1] / dur, 0.0), 1.0);
      for (int i = threadIdx.x; i < sp.rows - 1; i += kThreads) {
        const double si = lg_pos(sp, i), sn = lg_pos(sp, i + 1);
        if (si <= ps && ps < sn) atomicMax(&label[0], i);
        if (si <= pe && pe < sn) atomicMax(&label[1], i);
      }
      __syncthreads();
      if (threadIdx.x == 0) {
        framestps[2 * b] = label[0] < 0 ? 0 : label[0];
        framestps[2 * b + 1] = label[1] < 0 ? T - 1 : label[1];
      }
    } else if (threadIdx.x == 0 && framestps) {
#pragma unroll
      for (int q = 0; q < 2; ++q) {                           // int(x) if int(x) < SAMPLE_LEN else SAMPLE_LEN - 1 (charades.py:178)
        const int f = (int)timestamps[2 * b + q];
        framestps[2 * b + q] = f < T ? f : T - 1;
      }
    }
    if (threadIdx.x == 0) {
      nfeats[b] = sp.nf;
      if (spos_out) spos_out[b] = sp.spos;
    }
  }
  __syncthreads();
  const int d4 = D / 4, per_wg = kRowsPerWg * d4;
  const float4* rb = reinterpret_cast<const float4*>(raw) + (size_t)r0 * d4;
  ST* ob = out + (size_t)b * T * D;
  for (int base = threadIdx.x; base < per_wg; base += kUnroll * kThreads) {
    float4 acc[kUnroll];
    int2 w[kUnroll];
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {                    // first row of every window: all loads issued before any add
      const int idx = base + u * kThreads, r = idx / d4, k = idx - r * d4;
      acc[u] = make_float4(0.f, 0.f, 0.f, 0.f);
      w[u] = idx < per_wg && t0 + r < T ? win[r] : make_int2(0, 0);
      if (w[u].y > 0) acc[u] = rb[(size_t)w[u].x * d4 + k];
    }
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      if (w[u].y > 1) {
        const int idx = base + u * kThreads, k = idx - (idx / d4) * d4;
        const float4* p = rb + (size_t)w[u].x * d4 + k;
        for (int j = 1; j < w[u].y; ++j) {                    // sequential fp32 sum in row order
          const float4 x = p[(size_t)j * d4];
          acc[u].x += x.x; acc[u].y += x.y; acc[u].z += x.z; acc[u].w += x.w;
        }
        const float c = (float)w[u].y;                        // one correctly rounded division (not a multiply by 1/c)
        acc[u].x = acc[u].x / c; acc[u].y = acc[u].y / c; acc[u].z = acc[u].z / c; acc[u].w = acc[u].w / c;
      }
    }
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      const int idx = base + u * kThreads, r = idx / d4, k = idx - r * d4, t = t0 + r;
      if (idx < per_wg && t < T) st4(ob + (size_t)t * D + 4 * k, acc[u]);
    }
  }
}

// Sequence_mask(T, [st, et]): ones on [max(0,st), min(et, T-1)] inclusive (charades.py:12-18)
__device__ __forceinline__ int seq_mask(int t, int st, int et, int T) { return (t >= max(0, st) && t <= min(et, T - 1)) ? 1 : 0; }

__global__ __launch_bounds__(kThreads) void sequence_masks_kernel(
    const int* __restrict__ nfeats, const int* __restrict__ spans, int* __restrict__ vm, int* __restrict__ tl,
    int* __restrict__ fm, int* __restrict__ bm, int B, int T) {
  const int idx = blockIdx.x * kThreads + threadIdx.x;
  if (idx >= B * T) return;
  const int b = idx / T, t = idx % T;
  const int nf = nfeats[b], s = spans[2 * b], e = spans[2 * b + 1];
  if (vm) vm[idx] = seq_mask(t, 0, nf, T);                    // video_mask     = [0, nfeats]   (charades.py:167)
  if (tl) tl[idx] = seq_mask(t, s, e, T);                     // temporal_labels = framestamps  (:168)
  if (fm) fm[idx] = seq_mask(t, 0, s, T);                     // fore_mask      = [0, start]    (:169)
  if (bm) bm[idx] = seq_mask(t, e, nf, T);                    // back_mask      = [end, nfeats] (:170)
}

// span_pred: row i of the matrix is m[i][j] = j >= i ? fl(start_i + end_j) : 0 (triu zero-fills the lower triangle, which
// takes part in the max).  torch.max returns the FIRST maximal index along a dimension: strict '>' in increasing j, then in
// increasing i.  The sums are formed exactly as the reference forms them (one fp32 add per (i, j)): ties created by rounding
// must resolve the same way, so the O(T^2) walk is kept -- 64 x 128^2 adds is nothing.
__global__ __launch_bounds__(kThreads) void span_pred_kernel(const float* __restrict__ start, const float* __restrict__ end,
                                                            long long* __restrict__ pred, float* __restrict__ score, int B, int T) {
  extern __shared__ float sh[];                               // end row [T]
  __shared__ float wbest[kThreads / kWave];
  __shared__ int wi[kThreads / kWave], wj[kThreads / kWave];
  const int b = blockIdx.x, tid = threadIdx.x;
  for (int j = tid; j < T; j += kThreads) sh[j] = end[(size_t)b * T + j];
  __syncthreads();
  float best = -INFINITY; int bi = 0x7fffffff, bj = 0;
  for (int i = tid; i < T; i += kThreads) {                   // rows in increasing i per thread
    const float si = start[(size_t)b * T + i];
    float rb = i == 0 ? si + sh[0] : 0.f; int rj = 0;
    for (int j = 1; j < T; ++j) {
      const float v = j >= i ? si + sh[j] : 0.f;
      if (v > rb) { rb = v; rj = j; }
    }
    if (rb > best) { best = rb; bi = i; bj = rj; }
  }
  // (value, row) argmax with the smaller row winning ties: across the wave, then across the waves
#pragma unroll
  for (int off = 1; off < kWave; off <<= 1) {
    const float ob = __shfl_xor(best, off, kWave); const int oi = __shfl_xor(bi, off, kWave), oj = __shfl_xor(bj, off, kWave);
    if (ob > best || (ob == best && oi < bi)) { best = ob; bi = oi; bj = oj; }
  }
  if ((tid & (kWave - 1)) == 0) { wbest[tid / kWave] = best; wi[tid / kWave] = bi; wj[tid / kWave] = bj; }
  __syncthreads();
  if (tid == 0) {
    for (int u = 1; u < kThreads / kWave; ++u)
      if (wbest[u] > best || (wbest[u] == best && wi[u] < bi)) { best = wbest[u]; bi = wi[u]; bj = wj[u]; }
    pred[2 * b] = bi; pred[2 * b + 1] = bj; score[b] = best;
  }
}

int check_ptrs(const char* fn, std::initializer_list<const void*> ptrs) {
  for (const void* p : ptrs) {
    if (!p) return set_error(TSG_E_NULL, "%s: NULL pointer argument", fn);
    if (!aligned16(p)) return set_error(TSG_E_ALIGN, "%s: pointer %p is not 16-byte aligned", fn, p);
  }
  return 0;
}

// one launch of sample_clips_kernel; the entry points below have checked the arguments
int launch_sample_clips(const void* raw, const int64_t* offsets, const double* timestamps, const double* durations, int mode,
                        int train, uint64_t seed, const int32_t* spos_in, void* out, int32_t* nfeats, int32_t* framestps,
                        int32_t* spos_out, int B, int T, int D, int dtype, void* stream, const char* fn) {
  const int tiles = cdiv(T, kRowsPerWg);
  if ((long long)B * tiles > 0x7fffffffLL) return set_error(TSG_E_SHAPE, "%s: B=%d T=%d: grid too large", fn, B, T);
  const hipStream_t st = static_cast<hipStream_t>(stream);
  if (dtype == TSG_BF16)
    hipLaunchKernelGGL(sample_clips_kernel<bf16_t>, dim3(B * tiles), dim3(kThreads), 0, st, (const float*)raw,
                       (const long long*)offsets, timestamps, durations, mode, train, (unsigned long long)seed, spos_in,
                       (bf16_t*)out, nfeats, framestps, spos_out, T, D, tiles);
  else
    hipLaunchKernelGGL(sample_clips_kernel<float>, dim3(B * tiles), dim3(kThreads), 0, st, (const float*)raw,
                       (const long long*)offsets, timestamps, durations, mode, train, (unsigned long long)seed, spos_in,
                       (float*)out, nfeats, framestps, spos_out, T, D, tiles);
  return check_launch(fn);
}

}  // namespace
}  // namespace tsg

using namespace tsg;

extern "C" int tsg_moment_translate(const void* video, const int32_t* spans, const int32_t* nfeats, const int32_t* cropin,
                                    uint64_t seed, void* out, int32_t* new_spans, int B, int T, int D, int dtype, void* stream) {
  const char* fn = "tsg_moment_translate";
  int rc = check_ptrs(fn, {video, spans, nfeats, out, new_spans});
  if (rc) return rc;
  if (dtype != TSG_F32) return set_error(TSG_E_DTYPE, "%s: dtype %d not supported (fp32 only)", fn, dtype);
  if (B <= 0 || T <= 0 || D <= 0) return set_error(TSG_E_SHAPE, "%s: non-positive dimension B=%d T=%d D=%d", fn, B, T, D);
  if (D % 4) return set_error(TSG_E_ALIGN, "%s: D=%d must be a multiple of 4", fn, D);
  if (video == out) return set_error(TSG_E_SHAPE, "%s: in-place operation is not supported", fn);
  const int tiles = cdiv(T, kRowsPerWg);
  hipLaunchKernelGGL(moment_translate_kernel, dim3(B * tiles), dim3(kThreads), 0, static_cast<hipStream_t>(stream),
                     (const float*)video, spans, nfeats, cropin, (unsigned long long)seed, (float*)out, new_spans, B, T, D, tiles);
  return check_launch(fn);
}

extern "C" int tsg_pool_clips(const void* raw, const int64_t* offsets, const double* timestamps, void* out, int32_t* nfeats,
                              int32_t* framestps, int B, int T, int D, int dtype, void* stream) {
  const char* fn = "tsg_pool_clips";
  int rc = check_ptrs(fn, {raw, offsets, out, nfeats});
  if (rc) return rc;
  if (dtype != TSG_F32) return set_error(TSG_E_DTYPE, "%s: dtype %d not supported (fp32 only)", fn, dtype);
  if (B <= 0 || T <= 0 || D <= 0) return set_error(TSG_E_SHAPE, "%s: non-positive dimension B=%d T=%d D=%d", fn, B, T, D);
  if (D % 4) return set_error(TSG_E_ALIGN, "%s: D=%d must be a multiple of 4", fn, D);
  if ((timestamps == nullptr) != (framestps == nullptr)) return set_error(TSG_E_NULL, "%s: timestamps and framestps go together", fn);
  return launch_sample_clips(raw, offsets, timestamps, nullptr, TSG_SAMPLE_PAIR, 0, 0, nullptr, out, nfeats, framestps, nullptr,
                             B, T, D, dtype, stream, fn);
}

extern "C" int tsg_sample_clips(const void* raw, const int64_t* offsets, const double* timestamps, const double* durations,
                                int mode, int train, uint64_t seed, const int32_t* spos, void* out, int32_t* nfeats,
                                int32_t* framestps, int32_t* spos_out, int B, int T, int D, int dtype, void* stream) {
  const char* fn = "tsg_sample_clips";
  int rc = check_ptrs(fn, {raw, offsets, out, nfeats});
  if (rc) return rc;
  for (const void* p : {(const void*)timestamps, (const void*)durations, (const void*)spos, (const void*)framestps, (const void*)spos_out})
    if (p && !aligned16(p)) return set_error(TSG_E_ALIGN, "%s: pointer %p is not 16-byte aligned", fn, p);
  if (mode < TSG_SAMPLE_PAIR || mode > TSG_SAMPLE_LG) return set_error(TSG_E_SHAPE, "%s: unknown mode %d", fn, mode);
  if (dtype != TSG_F32 && dtype != TSG_BF16) return set_error(TSG_E_DTYPE, "%s: dtype %d not supported (fp32 or bf16)", fn, dtype);
  if (B <= 0 || T <= 0 || D <= 0) return set_error(TSG_E_SHAPE, "%s: non-positive dimension B=%d T=%d D=%d", fn, B, T, D);
  if (T > kMaxSampleT) return set_error(TSG_E_SHAPE, "%s: T=%d > %d", fn, T, kMaxSampleT);
  if (D % 4) return set_error(TSG_E_ALIGN, "%s: D=%d must be a multiple of 4", fn, D);
  if ((timestamps == nullptr) != (framestps == nullptr)) return set_error(TSG_E_NULL, "%s: timestamps and framestps go together", fn);
  const bool need_dur = mode == TSG_SAMPLE_F2S || mode == TSG_SAMPLE_F2S_114 || mode == TSG_SAMPLE_LG;
  if (need_dur && !durations) return set_error(TSG_E_NULL, "%s: mode %d needs durations", fn, mode);
  if (mode == TSG_SAMPLE_LG && !timestamps) return set_error(TSG_E_NULL, "%s: mode %d (LG) needs timestamps and framestps", fn, mode);
  return launch_sample_clips(raw, offsets, timestamps, durations, mode, train, seed, spos, out, nfeats, framestps, spos_out,
                             B, T, D, dtype, stream, fn);
}

extern "C" int tsg_sequence_masks(const int32_t* nfeats, const int32_t* spans, int32_t* video_mask, int32_t* temporal_labels,
                                  int32_t* fore_mask, int32_t* back_mask, int B, int T, void* stream) {
  const char* fn = "tsg_sequence_masks";
  int rc = check_ptrs(fn, {nfeats, spans});
  if (rc) return rc;
  if (B <= 0 || T <= 0) return set_error(TSG_E_SHAPE, "%s: non-positive dimension B=%d T=%d", fn, B, T);
  hipLaunchKernelGGL(sequence_masks_kernel, dim3(cdiv(B * T, kThreads)), dim3(kThreads), 0, static_cast<hipStream_t>(stream),
                     nfeats, spans, video_mask, temporal_labels, fore_mask, back_mask, B, T);
  return check_launch(fn);
}

extern "C" int tsg_span_pred(const void* start, const void* end, int64_t* pred, void* score, int B, int T, int dtype, void* stream) {
  const char* fn = "tsg_span_pred";
  int rc = check_ptrs(fn, {start, end, pred, score});
  if (rc) return rc;
  if (dtype != TSG_F32) return set_error(TSG_E_DTYPE, "%s: dtype %d not supported (fp32 only)", fn, dtype);
  if (B <= 0 || T <= 0) return set_error(TSG_E_SHAPE, "%s: non-positive dimension B=%d T=%d", fn, B, T);
  if (T > 16384) return set_error(TSG_E_LDS, "%s: T=%d > 16384", fn, T);
  hipLaunchKernelGGL(span_pred_kernel, dim3(B), dim3(kThreads), sizeof(float) * T, static_cast<hipStream_t>(stream),
                     (const float*)start, (const float*)end, (long long*)pred, (float*)score, B, T);
  return check_launch(fn);
}
