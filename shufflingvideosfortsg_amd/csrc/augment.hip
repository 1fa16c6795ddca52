// The crop family of the reference's data augmentation (DataAugmentForTSG, grounding/dataset/data_augment.py:5-156) for a whole
// batch in one launch (gfx950):
//   tsg_moment_augment  gt_translate / gt_crop / prot_gt_crop / gt_cropout and the two-candidate modes 'all' and None.
//
// Every workgroup works on one sample b and a tile of kRowsPerWg output rows, in two stages:
//   (a) draw: the sample's plan (op, a, b, c) -- the choices aug_data makes, in its order and over its inclusive random.randint
//       ranges -- from a counter-based hash of (seed, b, draw slot).  Each workgroup of a sample recomputes the same plan (a few
//       dozen scalar operations); the tile-0 workgroup writes it out with the new span and nfeats.  A caller-given plan skips it.
//   (b) apply: out[b, t] = video[b, src(t)] or a zero row, 16-byte loads and stores of raw elements (fp32 and bf16 alike: the
//       augmentation only moves rows, it never converts).
// Like tsg_moment_translate it is bound by HBM: each output row is read once (or not at all: zero rows) and written once.
#include "tsg_common.h"

namespace tsg {
namespace {

constexpr int kThreads = 256;
constexpr int kRowsPerWg = 8;                 // output rows per workgroup; all loads of a thread issued before its stores
constexpr int kUnroll = 8;

enum : int { kOpIdentity = 0, kOpTranslate = 1, kOpCrop = 2, kOpCropout = 3 };
// draw slots: each choice has its own counter, so a plan does not depend on which earlier draws were taken
enum : int { kSlotGate = 0, kSlotFn = 1, kSlotWidth = 2, kSlotStart = 3, kSlotPick = 4, kSlotFbWidth = 5, kSlotFbStart = 6 };
constexpr double kProtectedRatio = 0.2, kMinWidthRatio = 0.2, kMaxWidthRatio = 0.5;   // data_augment.py:9, aug_data defaults (:28)

__device__ __forceinline__ unsigned long long splitmix64(unsigned long long x) {
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}

__device__ __forceinline__ unsigned long long aug_hash(unsigned long long seed, int b, int slot) {
  return splitmix64(seed ^ (0xD1B54A32D192ED03ull * (unsigned long long)(b + 1)) ^
                    (0xA0761D6478BD642Full * (unsigned long long)(slot + 1)));
}

// random.randint(lo, hi): uniform over [lo, hi] INCLUSIVE (multiply-high of the hash's upper 32 bits)
__device__ __forceinline__ int draw_int(unsigned long long seed, int b, int slot, int lo, int hi) {
  if (hi <= lo) return lo;
  return lo + (int)(((aug_hash(seed, b, slot) >> 32) * (unsigned long long)(hi - lo + 1)) >> 32);
}

// np.random.rand(): [0, 1) with 53 bits
__device__ __forceinline__ double draw_unit(unsigned long long seed, int b, int slot) {
  return (double)(aug_hash(seed, b, slot) >> 11) * 0x1.0p-53;
}

// np.ceil(x * ratio) of an integer x, in double as numpy forms it (ceil(-0.2) = -0 -> 0)
__device__ __forceinline__ int ceil_ratio(int x, double ratio) { return (int)ceil((double)x * ratio); }

struct Plan { int op, a, b, c; };

// gt_moment_crop with fresh draws (data_augment.py:38-63): width in [ceil(.2 len), ceil(.5 len)], start in [s, e - w + 1]
__device__ __forceinline__ Plan draw_crop(unsigned long long seed, int b, int s, int e, int slot_w, int slot_s) {
  const int len = e - s + 1;
  if (len <= 1) return {kOpIdentity, 0, 0, 0};
  const int w = draw_int(seed, b, slot_w, ceil_ratio(len, kMinWidthRatio), ceil_ratio(len, kMaxWidthRatio));
  return {kOpCrop, w, draw_int(seed, b, slot_s, s, e - w + 1), 0};
}

// protected_gt_moment_crop (:65-93): the same inside [s + ceil(.2 len), e - ceil(.2 len)]; that interval's "length" pe - ps
// is -1 or 0 for moments of 2-3 clips: width 0, an applied crop that deletes nothing
__device__ __forceinline__ Plan draw_prot_crop(unsigned long long seed, int b, int s, int e) {
  const int len = e - s + 1;
  if (len <= 1) return {kOpIdentity, 0, 0, 0};
  const int c = ceil_ratio(len, kProtectedRatio), ps = s + c, pe = e - c;
  const int w = draw_int(seed, b, kSlotWidth, ceil_ratio(pe - ps, kMinWidthRatio), ceil_ratio(pe - ps, kMaxWidthRatio));
  return {kOpCrop, w, draw_int(seed, b, kSlotStart, ps, pe - w + 1), 0};
}

// gt_moment_cropout (:95-133): overwrite w rows inside the protected moment with w rows from outside it; falls back to a crop
// with fresh draws when w <= 0 and to a crop with the drawn (w, cropout start) when no outside block fits
__device__ __forceinline__ Plan draw_cropout(unsigned long long seed, int b, int s, int e, int nf) {
  const int len = e - s + 1;
  if (len <= 1) return {kOpIdentity, 0, 0, 0};
  const int c = ceil_ratio(len, kProtectedRatio);
  const int psl = s - c, psr = s + c, pel = e - c, per = e + c;
  const int w = draw_int(seed, b, kSlotWidth, ceil_ratio(pel - psr, kMinWidthRatio), ceil_ratio(pel - psr, kMaxWidthRatio));
  if (w <= 0) return draw_crop(seed, b, s, e, kSlotFbWidth, kSlotFbStart);
  const int out_start = draw_int(seed, b, kSlotStart, psr, pel - w + 1);
  const int n_left = psl >= w ? psl : 0;                      // candidates [0, psl - 1]
  const int n_right = nf - 1 - per >= w ? nf - w - per : 0;   // candidates [per, nf - w - 1]
  if (n_left + n_right == 0) return {kOpCrop, w, out_start, 0};
  const int k = n_left + n_right > 1 ? draw_int(seed, b, kSlotPick, 0, n_left + n_right - 1) : 0;
  return {kOpCropout, w, out_start, k < n_left ? k : per + (k - n_left)};
}

// gt_moment_translate (:135-156): insert position in [0, nfeats - len]; moments of length <= 1 or covering every clip: no-op
__device__ __forceinline__ Plan draw_translate(unsigned long long seed, int b, int s, int e, int nf) {
  const int len = e - s + 1;
  if (len <= 1 || len >= nf) return {kOpIdentity, 0, 0, 0};
  return {kOpTranslate, draw_int(seed, b, kSlotWidth, 0, nf - len), 0, 0};
}

// aug_data (:28-36): the gate np.random.rand() > p skips (p <= 0: never applied, p >= 1: always), then one of the mode's
// candidate functions (random.randint(0, 1) for two)
__device__ __forceinline__ Plan draw_plan(int mode, double p, unsigned long long seed, int b, int s, int e, int nf) {
  const bool apply = p >= 1.0 || (p > 0.0 && !(draw_unit(seed, b, kSlotGate) > p));
  if (!apply) return {kOpIdentity, 0, 0, 0};
  int fn = mode;
  if (mode == TSG_AUG_ALL) fn = draw_int(seed, b, kSlotFn, 0, 1) ? TSG_AUG_CROPOUT : TSG_AUG_PROT_CROP;
  else if (mode == TSG_AUG_DEFAULT) fn = draw_int(seed, b, kSlotFn, 0, 1) ? TSG_AUG_CROPOUT : TSG_AUG_CROP;
  switch (fn) {
    case TSG_AUG_TRANSLATE: return draw_translate(seed, b, s, e, nf);
    case TSG_AUG_CROP: return draw_crop(seed, b, s, e, kSlotWidth, kSlotStart);
    case TSG_AUG_PROT_CROP: return draw_prot_crop(seed, b, s, e);
    default: return draw_cropout(seed, b, s, e, nf);
  }
}

// The plan as a row map.  Every field is clamped to [0, T] so that any plan (caller-given ones included) reads only rows of
// sample b; src() may still return rows >= T, which read as zero rows.
struct RowMap {
  int op, s, len, nf, w, at, from;
  __device__ __forceinline__ int src(int t) const {
    switch (op) {
      case kOpTranslate: {                                    // [0, at): gap-closed rows, [at, at+len): the moment, then the rest
        if (t >= at && t < at + len) return s + (t - at);     // (a moment ending at or past nf: the gap-closed rows are [0, s),
        const int i = t < at ? t : t - len;                   // as tsg_moment_translate's translate_src)
        if (i < s) return i;
        return i < nf - len ? i + len : -1;
      }
      case kOpCrop: return t < at ? t : t + w;                // rows [at, at+w) deleted, the rest (zero padding too) shifts left
      case kOpCropout: return t >= at && t < at + w ? from + (t - at) : t;
      default: return t;
    }
  }
};

__device__ __forceinline__ int clamp_t(int v, int T) { return min(max(v, 0), T); }

__global__ __launch_bounds__(kThreads) void moment_augment_kernel(
    const uint4* __restrict__ video, const int* __restrict__ spans, const int* __restrict__ nfeats, int mode, double p,
    unsigned long long seed, const int* __restrict__ plan_in, int* __restrict__ plan_out, uint4* __restrict__ out,
    int* __restrict__ new_spans, int* __restrict__ new_nfeats, int T, int row_vecs, int tiles) {
  const int b = blockIdx.x / tiles, t0 = (blockIdx.x % tiles) * kRowsPerWg;
  const int s = spans[2 * b], e = spans[2 * b + 1], nf = nfeats[b], len = e - s + 1;
  const Plan pl = plan_in ? Plan{plan_in[4 * b], plan_in[4 * b + 1], plan_in[4 * b + 2], plan_in[4 * b + 3]}
                          : draw_plan(mode, p, seed, b, s, e, nf);
  RowMap m{kOpIdentity, s, len, nf, 0, 0, 0};
  int ns = s, ne = e, nnf = nf;
  if (pl.op == kOpTranslate && len > 1 && len < nf) {
    m.op = kOpTranslate;
    m.at = min(max(pl.a, 0), max(nf - len, 0));
    ns = m.at; ne = m.at + len - 1;
  } else if (pl.op == kOpCrop) {
    m.op = kOpCrop; m.w = clamp_t(pl.a, T); m.at = clamp_t(pl.b, T);
    ne = e - m.w; nnf = nf - m.w;                             // the reference's arithmetic (:59-61), whatever was deleted
  } else if (pl.op == kOpCropout) {
    m.op = kOpCropout; m.w = clamp_t(pl.a, T); m.at = clamp_t(pl.b, T); m.from = clamp_t(pl.c, T);
  }
  if (blockIdx.x % tiles == 0 && threadIdx.x == 0) {
    new_spans[2 * b] = ns;
    new_spans[2 * b + 1] = ne;
    new_nfeats[b] = nnf;
    if (plan_out) {
      plan_out[4 * b] = pl.op; plan_out[4 * b + 1] = pl.a; plan_out[4 * b + 2] = pl.b; plan_out[4 * b + 3] = pl.c;
    }
  }
  const int per_wg = kRowsPerWg * row_vecs;
  const uint4* vb = video + (size_t)b * T * row_vecs;
  uint4* ob = out + (size_t)b * T * row_vecs;
  for (int base = threadIdx.x; base < per_wg; base += kUnroll * kThreads) {
    uint4 v[kUnroll];
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      const int idx = base + u * kThreads, r = idx / row_vecs, k = idx - r * row_vecs, t = t0 + r;
      v[u] = make_uint4(0u, 0u, 0u, 0u);
      if (idx < per_wg && t < T) {
        const int src = m.src(t);
        if (src >= 0 && src < T) v[u] = vb[(size_t)src * row_vecs + k];
      }
    }
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      const int idx = base + u * kThreads, r = idx / row_vecs, k = idx - r * row_vecs, t = t0 + r;
      if (idx < per_wg && t < T) ob[(size_t)t * row_vecs + k] = v[u];
    }
  }
}

int check_ptrs(const char* fn, std::initializer_list<const void*> ptrs, bool optional) {
  for (const void* p : ptrs) {
    if (!p) {
      if (optional) continue;
      return set_error(TSG_E_NULL, "%s: NULL pointer argument", fn);
    }
    if (!aligned16(p)) return set_error(TSG_E_ALIGN, "%s: pointer %p is not 16-byte aligned", fn, p);
  }
  return 0;
}

}  // namespace
}  // namespace tsg

using namespace tsg;

extern "C" int tsg_moment_augment(const void* video, const int32_t* spans, const int32_t* nfeats, int mode, double aug_percentage,
                                  uint64_t seed, const int32_t* plan, int32_t* plan_out, void* out, int32_t* new_spans,
                                  int32_t* new_nfeats, int B, int T, int D, int dtype, void* stream) {
  const char* fn = "tsg_moment_augment";
  int rc = check_ptrs(fn, {video, spans, nfeats, out, new_spans, new_nfeats}, false);
  if (!rc) rc = check_ptrs(fn, {plan, plan_out}, true);
  if (rc) return rc;
  if (dtype != TSG_F32 && dtype != TSG_BF16) return set_error(TSG_E_DTYPE, "%s: dtype %d not supported (fp32 or bf16)", fn, dtype);
  if (B <= 0 || T <= 0 || D <= 0) return set_error(TSG_E_SHAPE, "%s: non-positive dimension B=%d T=%d D=%d", fn, B, T, D);
  const int per_vec = dtype == TSG_BF16 ? 8 : 4;             // elements per 16-byte vector
  if (D % per_vec) return set_error(TSG_E_ALIGN, "%s: D=%d must be a multiple of %d", fn, D, per_vec);
  if (video == out) return set_error(TSG_E_SHAPE, "%s: in-place operation is not supported", fn);
  if (mode < TSG_AUG_TRANSLATE || mode > TSG_AUG_DEFAULT) return set_error(TSG_E_SHAPE, "%s: unknown mode %d", fn, mode);
  const int tiles = cdiv(T, kRowsPerWg);
  if ((long long)B * tiles > 0x7fffffffLL) return set_error(TSG_E_SHAPE, "%s: B=%d T=%d: grid too large", fn, B, T);
  launch_timed(moment_augment_kernel, dim3(B * tiles), dim3(kThreads), 0, static_cast<hipStream_t>(stream),
               static_cast<const uint4*>(video), spans, nfeats, mode, aug_percentage, (unsigned long long)seed, plan, plan_out,
               static_cast<uint4*>(out), new_spans, new_nfeats, T, D / per_vec, tiles);
  return check_launch(fn);
}
