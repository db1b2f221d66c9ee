// Object-level matching: per class, which connected region of the prediction overlaps which connected region of the truth with an IoU
// above a threshold of at least 1/2 (the definition is the comment block of sg_object_match in include/segearth_hip.h).  A match needs
// I > |p| / 2, so the partner of a predicted object p is the strict MAJORITY among the true objects of p's class that p's pixels lie in:
// it is found by a mergeable Boyer-Moore summary per predicted root, with no hash table, no sort and no cap on the number of objects.
// Per call one kernel, then per launch sequence of up to SG_SIEVE_GROUP images (descriptors in the launch arguments, sieve_label.h):
//   object_prepare  : G' = the truth after reduce_zero_label as int64, so that the labelling kernels run on it as they are; the
//                     intersection counters and the truth's match marks zeroed.
//   sieve_local / sieve_merge / sieve_flatten on P (which also zeroes the summaries) and on G': parentP, areaP, parentG, areaG.
//   object_vote     : one 64-bit word per predicted root, (candidate true root : 32, counter : 32).  A pixel whose predicted and true
//                     regions are objects of one class votes for its true root.  Votes merge before they touch memory: the OM_RUN
//                     consecutive pixels of a lane, then equal (predicted root, true root) pairs across the wave by leader match; what
//                     is left goes through the workgroup's LDS cache (a workgroup sweeps OM_CHUNKS chunks of 2048 pixels and keeps its
//                     merged pairs until it ends) and merges into the word by a 64-bit compare-and-swap loop: equal candidates add
//                     their counters, unequal ones leave the larger counter minus the smaller under the larger one's candidate.  The summary of a multiset is
//                     mergeable in any order (Agarwal et al., "Mergeable Summaries", PODS 2012: Misra-Gries with one counter): if a
//                     strict majority exists it is the final candidate with a positive counter, whatever the order.  If none exists
//                     the candidate is arbitrary and object_decide rejects it whatever it is.
//   object_verify   : a pixel whose true root is the candidate of its predicted root adds to the 32-bit intersection counter of the
//                     predicted root, merged the same way: I = |p n g| exactly.
//   object_decide   : over the root pixels.  A predicted object adds to row 1, a true object to row 2; a predicted object whose candidate
//                     passes I * den > num * (|p| + |g| - I) adds to row 0 and floor(I * 2^24 / U) to row 3 and marks both roots.  K-wide
//                     LDS bins per workgroup (32-bit for rows 0 to 2, 64-bit for row 3), one 64-bit add per non-zero bin per workgroup.
//   object_map      : only with match_map: the byte of every pixel from the marks of its two roots.
// The retry of the compare-and-swap is lock-free (it repeats only when another thread's merge went through), so no workgroup waits for
// another.  Integers and integer atomics only; every value that reaches an output is independent of the arrival order (the candidate of
// an object WITHOUT a majority is not, and never passes the test); nothing visits the host; labels and gt are only read.
#include "sieve_label.h"

namespace sg {

constexpr int OM_MAX_K = LM_MAX_K;
constexpr int OM_RUN = SV_RUN;                                        // consecutive pixels per lane of object_vote / object_verify
constexpr int OM_MAX_DEN = 1 << 20;
constexpr int OM_SQ_SHIFT = 24;                                       // row 3 counts IoU in steps of 2^-24, as SG_REGION_SCORE_Q
constexpr int OM_CHUNKS = 16;                                         // chunks of SV_PIX pixels a workgroup of object_vote sweeps
constexpr int OM_SLOT_BITS = 6, OM_SLOTS = 1 << OM_SLOT_BITS;         // the workgroup's list and its cache; one lane of a wave per slot
static_assert(OM_RUN <= 15, "a run length is summed from four ballots");

struct ObjectRule { long long min_area, skip_label; int use_skip, K, ignore_index; };

// a region of value v and area a is an object (of class v); truth: the ignored value is none
template <bool TRUTH> __device__ __forceinline__ bool object_is(const ObjectRule& ru, int64_t v, int a) {
  if ((uint64_t)v >= (uint64_t)ru.K || (long long)a < ru.min_area) return false;
  if (ru.use_skip && v == ru.skip_label) return false;
  return !TRUTH || v != (int64_t)ru.ignore_index;
}

// Flat over the pixels of the call: the images lie back to back, so a pixel's place in gt is its place in the workspace.
template <typename T>
__global__ __launch_bounds__(256) void object_prepare_kernel(const T* __restrict__ gt, int rzl, int64_t total, int64_t* __restrict__ gprime,
                                                             uint32_t* __restrict__ inter, uint8_t* __restrict__ mark_g) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    gprime[i] = lm_value(gt, i, rzl);
    inter[i] = 0u;
    mark_g[i] = 0;
  }
}

// The merge of (key, 1) over the OM_RUN consecutive pixels of every lane and over the wave: equal neighbours of a lane become one (key,
// length) pair; slot by slot the wave combines by leader match (the ballot of the lanes on the first unserved lane's key, four ballots for
// the sum of their lengths) and the leader sends (key, sum); after three rounds, once a round matches fewer than 4 lanes, every lane
// that is left sends its own pair: those are mostly distinct keys.  key < 0: no vote.  The loop is wave-uniform.
template <typename Send>
__device__ __forceinline__ void object_merge_run(const long long (&key)[OM_RUN], int lane, Send send) {
  int len[OM_RUN];
  len[OM_RUN - 1] = 1;
#pragma unroll
  for (int j = OM_RUN - 2; j >= 0; --j) len[j] = key[j] == key[j + 1] ? len[j + 1] + 1 : 1;
#pragma unroll
  for (int j = 0; j < OM_RUN; ++j) {
    bool act = key[j] >= 0 && (j == 0 || key[j] != key[j - 1]);       // the head of a run of votes
    unsigned long long rem = __ballot(act);
    int rounds = 0;
    while (rem != 0ull) {
      const int src = __ffsll((long long)rem) - 1;
      const int lo = __builtin_amdgcn_readlane((int)(uint32_t)key[j], src), hi = __builtin_amdgcn_readlane((int)(key[j] >> 32), src);
      const long long lk = ((long long)hi << 32) | (long long)(uint32_t)lo;
      const bool m = act && key[j] == lk;
      const unsigned long long mm = __ballot(m);
      int total = 0;                                                   // the sum of len (<= OM_RUN: 4 bits) over the matching lanes
#pragma unroll
      for (int b = 0; b < 4; ++b) total += __popcll(__ballot(m && ((len[j] >> b) & 1))) << b;
      if (lane == src) send(lk, (uint32_t)total);
      act = act && !m;
      rem &= ~mm;
      if (++rounds >= 3 && __popcll(mm) < 4) break;
    }
    if (act) send(key[j], (uint32_t)len[j]);
  }
}

// summary[p] <- merge(summary[p], (g, n)), n >= 1.  A word with counter 0 is empty.  The loop repeats only when the word changed between
// the read and the swap, that is when another thread's merge succeeded.
__device__ __forceinline__ void object_vote_merge(unsigned long long* word, uint32_t g, uint32_t n) {
  unsigned long long old = __hip_atomic_load(word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  for (;;) {
    const uint32_t og = (uint32_t)(old >> 32), on = (uint32_t)old;
    unsigned long long nw;
    if (on == 0u || og == g) nw = ((unsigned long long)g << 32) | (unsigned long long)(on + n);      // the counters of one object stay below 2^31
    else if (on >= n) nw = ((unsigned long long)og << 32) | (unsigned long long)(on - n);
    else nw = ((unsigned long long)g << 32) | (unsigned long long)(n - on);
    const unsigned long long seen = atomicCAS(word, old, nw);
    if (seen == old) return;
    old = seen;
  }
}

// The lane's OM_RUN consecutive pixels from i0 of the image: key[j] = (predicted root << 32 | true root) where both regions are objects
// of one class, else -1.  i < np is checked before any access; the roots' area entries are complete (kernel boundary).
__device__ __forceinline__ void object_pairs(const int64_t* __restrict__ lab, const int64_t* __restrict__ gp, const int32_t* __restrict__ PP,
                                             const int32_t* __restrict__ AP, const int32_t* __restrict__ PG, const int32_t* __restrict__ AG,
                                             const ObjectRule& ru, int64_t i0, int64_t np, long long (&key)[OM_RUN]) {
  int64_t v[OM_RUN], g[OM_RUN];
  int pr[OM_RUN], gr[OM_RUN];
#pragma unroll
  for (int j = 0; j < OM_RUN; ++j) {
    const bool in = i0 + j < np;
    v[j] = in ? lab[i0 + j] : -1;
    g[j] = in ? gp[i0 + j] : -2;
    pr[j] = in ? PP[i0 + j] : 0;
    gr[j] = in ? PG[i0 + j] : 0;
  }
#pragma unroll
  for (int j = 0; j < OM_RUN; ++j) {
    key[j] = -1;
    if (i0 + j >= np || v[j] != g[j]) continue;                        // the region's value is the pixel's
    if (!object_is<false>(ru, v[j], AP[pr[j]]) || !object_is<true>(ru, g[j], AG[gr[j]])) continue;
    key[j] = ((long long)pr[j] << 32) | (long long)gr[j];              // roots are below 2^31: the key is >= 0
  }
}

// A workgroup of object_vote sweeps OM_CHUNKS chunks of 2048 consecutive pixels of one image and keeps what it has merged in LDS until it
// ends: a large object then costs one global atomic per workgroup of 32 768 pixels, not one per wave.  (Atomics on one address pass one at
// a time, and a compare-and-swap that finds the word changed starts over: thousands of waves on one word cost their number SQUARED.)
struct ObjectBlocks { int prefix[SV_GROUP + 1]; };                    // workgroups of object_vote before the image

// Per chunk the waves append their merged (key, count) pairs to a list of OM_SLOTS entries (what does not fit is sent directly: those are
// mostly distinct keys); one wave then merges equal keys of the list by leader match and moves them into the cache: OM_SLOTS entries,
// direct-mapped by a hash of the predicted root.  An entry that finds its slot held by another key evicts it (the evicted pair is sent);
// of several entries of one round that want one slot the lowest lane takes it and the others are sent.  Only that one wave touches the
// cache, and LDS operations of one wave execute in order.
struct ObjectCache {
  long long list_key[OM_SLOTS], key[OM_SLOTS];
  uint32_t list_cnt[OM_SLOTS], cnt[OM_SLOTS];
  int claim[OM_SLOTS], n;
};

template <typename Send>
__device__ __forceinline__ void object_cache_merge(ObjectCache& c, int lane, Send send) {
  const int n = c.n < OM_SLOTS ? c.n : OM_SLOTS;
  bool act = lane < n;
  const long long k = act ? c.list_key[lane] : -1;
  uint32_t cnt = act ? c.list_cnt[lane] : 0u;
  bool lead = false;                                                   // this lane carries the sum of the lanes that hold its key
  unsigned long long rem = __ballot(act);
  int rounds = 0;
  while (rem != 0ull) {                                                // wave-uniform
    const int src = __ffsll((long long)rem) - 1;
    const int lo = __builtin_amdgcn_readlane((int)(uint32_t)k, src), hi = __builtin_amdgcn_readlane((int)(k >> 32), src);
    const long long lk = ((long long)hi << 32) | (long long)(uint32_t)lo;
    const bool m = act && k == lk;
    const unsigned long long mm = __ballot(m);
    uint32_t total = 0u;                                               // an entry counts at most 64 lanes x OM_RUN pixels: 10 bits
#pragma unroll
    for (int b = 0; b < 10; ++b) total += (uint32_t)__popcll(__ballot(m && ((cnt >> b) & 1u))) << b;
    if (lane == src) { cnt = total; lead = true; }
    act = act && !m;
    rem &= ~mm;
    if (++rounds >= 8 && __popcll(mm) < 2) break;
  }
  lead = lead || act;                                                  // what the loop left: entries of their own
  const int slot = (int)(((uint32_t)(k >> 32) * 2654435761u) >> (32 - OM_SLOT_BITS));
  volatile int* claim = c.claim;
  claim[lane] = 64;
  if (lead) atomicMin(&c.claim[slot], lane);
  if (lead) {
    if (claim[slot] == lane) {
      volatile long long* ck = c.key;
      volatile uint32_t* cc = c.cnt;
      if (ck[slot] == k) {
        cc[slot] = cc[slot] + cnt;
      } else {
        if (cc[slot] != 0u) send(ck[slot], cc[slot]);
        ck[slot] = k; cc[slot] = cnt;
      }
    } else {
      send(k, cnt);
    }
  }
}

template <bool VERIFY>
__global__ __launch_bounds__(256) void object_vote_kernel(const int64_t* __restrict__ labels, const int64_t* __restrict__ gprime, const SieveImages im,
                                                          const ObjectBlocks ob, const ObjectRule ru, const int32_t* __restrict__ parent_p,
                                                          const int32_t* __restrict__ area_p, const int32_t* __restrict__ parent_g,
                                                          const int32_t* __restrict__ area_g, unsigned long long* summary, uint32_t* inter) {
  __shared__ ObjectCache s_c;
  const int n = sieve_image_of(ob.prefix, im.n, (int)blockIdx.x);
  const int64_t np = (int64_t)im.h[n] * im.w[n], base0 = ((int64_t)blockIdx.x - ob.prefix[n]) * (OM_CHUNKS * SV_PIX);
  const int64_t wb = im.wbase[n];
  const int tid = threadIdx.x, lane = tid & 63;
  unsigned long long* S = summary + wb;
  uint32_t* I = inter + wb;
  auto send = [&](long long k, uint32_t cnt) {
    if constexpr (VERIFY) atomicAdd(I + (k >> 32), cnt);
    else object_vote_merge(S + (k >> 32), (uint32_t)k, cnt);
  };
  if (tid < OM_SLOTS) { s_c.key[tid] = -1; s_c.cnt[tid] = 0u; }
  for (int ch = 0; ch < OM_CHUNKS; ++ch) {                             // block-uniform
    const int64_t base = base0 + (int64_t)ch * SV_PIX;
    if (base >= np) break;
    if (tid == 0) s_c.n = 0;
    __syncthreads();                                                   // the list is free: the merging wave has passed this point too
    long long key[OM_RUN];
    object_pairs(labels + im.off[n], gprime + wb, parent_p + wb, area_p + wb, parent_g + wb, area_g + wb, ru, base + (int64_t)tid * OM_RUN, np, key);
    if constexpr (VERIFY) {                                            // summary is complete: written by the launch before this one
      long long pair[OM_RUN];
#pragma unroll
      for (int j = 0; j < OM_RUN; ++j) pair[j] = key[j];
#pragma unroll
      for (int j = 0; j < OM_RUN; ++j) {
        if (pair[j] < 0) continue;
        if (j > 0 && pair[j] == pair[j - 1]) { key[j] = key[j - 1]; continue; }    // the pair of the pixel before it: the same answer
        const unsigned long long w = S[pair[j] >> 32];
        if ((uint32_t)w == 0u || (uint32_t)(w >> 32) != (uint32_t)pair[j]) key[j] = -1;   // not the candidate of its predicted root
      }
    }
    object_merge_run(key, lane, [&](long long k, uint32_t cnt) {
      const int slot = atomicAdd(&s_c.n, 1);
      if (slot < OM_SLOTS) { s_c.list_key[slot] = k; s_c.list_cnt[slot] = cnt; }
      else send(k, cnt);
    });
    __syncthreads();
    if (tid < 64) object_cache_merge(s_c, lane, send);
  }
  __syncthreads();
  if (tid < OM_SLOTS && s_c.cnt[tid] != 0u) send(s_c.key[tid], s_c.cnt[tid]);
}

// Over the root pixels (the linear workgroups of the per-pixel kernels).  summary, inter and both area arrays are complete.  mark_p[root]
// = 1 matched, 2 unmatched object, 0 no object; mark_g[root] = 1 for the matched true objects only: a match is unique (2 num >= den), so
// each mark has one writer and needs no atomic.
__global__ __launch_bounds__(256) void object_decide_kernel(const int64_t* __restrict__ labels, const int64_t* __restrict__ gprime, const SieveImages im,
                                                            const ObjectRule ru, long long num, long long den, const int32_t* __restrict__ parent_p,
                                                            const int32_t* __restrict__ area_p, const int32_t* __restrict__ parent_g,
                                                            const int32_t* __restrict__ area_g, const unsigned long long* __restrict__ summary,
                                                            const uint32_t* __restrict__ inter, uint8_t* __restrict__ mark_p, uint8_t* mark_g,
                                                            unsigned long long* __restrict__ counts) {
  __shared__ uint32_t bins[3 * OM_MAX_K];
  __shared__ unsigned long long sq[OM_MAX_K];
  const int K = ru.K;
  for (int i = threadIdx.x; i < 3 * K; i += 256) bins[i] = 0u;
  for (int i = threadIdx.x; i < K; i += 256) sq[i] = 0ull;
  __syncthreads();
  const SievePixel p = sieve_pixel(im);
  const int64_t wb = im.wbase[p.n];
  const int64_t* lab = labels + im.off[p.n];
  const int64_t* gp = gprime + wb;
  for (int j = 0; j < SV_RUN; ++j) {
    const int64_t i = p.base + j * 256 + threadIdx.x;
    if (i >= p.np) break;
    if (parent_p[wb + i] == (int)i) {
      const int64_t v = lab[i];
      const int ap = area_p[wb + i];
      uint8_t mark = 0;
      if (object_is<false>(ru, v, ap)) {
        mark = 2;
        atomicAdd(&bins[K + (int)v], 1u);
        const unsigned long long w = summary[wb + i];
        if ((uint32_t)w != 0u) {                                       // a candidate: a true object of class v (only such pixels vote)
          const uint32_t g = (uint32_t)(w >> 32);
          const long long I = (long long)inter[wb + i], U = (long long)ap + (long long)area_g[wb + g] - I;
          if (I * den > num * U) {                                     // I < 2^31, den <= 2^20, U < 2^32: no overflow
            mark = 1;
            mark_g[wb + g] = 1;
            atomicAdd(&bins[(int)v], 1u);
            atomicAdd(&sq[(int)v], (unsigned long long)((I << OM_SQ_SHIFT) / U));
          }
        }
      }
      mark_p[wb + i] = mark;
    }
    if (parent_g[wb + i] == (int)i) {
      const int64_t g = gp[i];
      if (object_is<true>(ru, g, area_g[wb + i])) atomicAdd(&bins[2 * K + (int)g], 1u);
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < 3 * K; i += 256) {
    const uint32_t v = bins[i];
    if (v != 0u) atomicAdd(&counts[i], (unsigned long long)v);
  }
  for (int i = threadIdx.x; i < K; i += 256) {
    const unsigned long long v = sq[i];
    if (v != 0ull) atomicAdd(&counts[3 * K + i], v);
  }
}

__global__ __launch_bounds__(256) void object_map_kernel(const int64_t* __restrict__ gprime, const SieveImages im, const ObjectRule ru,
                                                         const int32_t* __restrict__ parent_p, const int32_t* __restrict__ parent_g,
                                                         const int32_t* __restrict__ area_g, const uint8_t* __restrict__ mark_p,
                                                         const uint8_t* __restrict__ mark_g, uint8_t* __restrict__ match_map) {
  const SievePixel p = sieve_pixel(im);
  const int64_t wb = im.wbase[p.n];
  uint8_t* out = match_map + im.off[p.n];
  for (int j = 0; j < SV_RUN; ++j) {
    const int64_t i = p.base + j * 256 + threadIdx.x;
    if (i >= p.np) return;
    const int gr = parent_g[wb + i];
    const int b = mark_g[wb + gr] ? 4 : (object_is<true>(ru, gprime[wb + i], area_g[wb + gr]) ? 8 : 0);
    out[i] = (uint8_t)((int)mark_p[wb + parent_p[wb + i]] + b);
  }
}

}  // namespace sg

using namespace sg;

extern "C" size_t sg_object_workspace_bytes(int64_t n_pixels_total) {
  if (n_pixels_total < 0) return 0;
  return (size_t)n_pixels_total * 36 + 2 * lm_plane_bytes(n_pixels_total);
}

extern "C" int sg_object_match(const int64_t* labels, const void* gt, int gt_format, const int32_t* image_hw, const int64_t* offset, int N, int K,
                               int connectivity, int64_t min_area, int64_t skip_label, int use_skip, int iou_num, int iou_den, int ignore_index,
                               int reduce_zero_label, int64_t* counts, uint8_t* match_map, void* workspace, size_t workspace_bytes, sg_stream s) {
  const char* who = "sg_object_match";
  SG_REQUIRE(labels && gt && image_hw && offset && counts && workspace, "%s: null pointer", who);
  SG_REQUIRE(gt_format == SG_GT_U8 || gt_format == SG_GT_I64, "%s: unknown ground-truth format %d", who, gt_format);
  SG_REQUIRE(K >= 1 && K <= OM_MAX_K, "%s: K=%d outside [1, %d] (the cap of sg_confusion_accumulate)", who, K, OM_MAX_K);
  SG_REQUIRE(connectivity == 4 || connectivity == 8, "%s: connectivity=%d is neither 4 nor 8", who, connectivity);
  SG_REQUIRE(min_area >= 1, "%s: min_area=%lld must be >= 1 (a region is an object when its area is at least it)", who, (long long)min_area);
  SG_REQUIRE(iou_num >= 1 && iou_num < iou_den && iou_den <= OM_MAX_DEN, "%s: the threshold %d / %d needs 1 <= num < den <= 2^20", who, iou_num, iou_den);
  SG_REQUIRE(2 * (int64_t)iou_num >= (int64_t)iou_den, "%s: the threshold %d / %d is below 1/2: the match would not be unique", who, iou_num, iou_den);
  int64_t total = 0;                                                   // per call: region roots index the call's pixels in 32 bits
  SG_TRY(lm_check_images(who, image_hw, offset, N, true, [](int) -> int { return SG_OK; }, &total));
  SG_REQUIRE(lm_aligned8(labels) && (gt_format == SG_GT_U8 || lm_aligned8(gt)) && lm_aligned8(counts) && lm_aligned8(workspace),
             "%s: int64 buffers and the workspace must be 8-byte aligned", who);
  const size_t need = sg_object_workspace_bytes(total);
  SG_REQUIRE(workspace_bytes >= need, "%s: workspace too small: %zu bytes given, %zu needed for %lld pixels", who, workspace_bytes, need,
             (long long)total);

  // workspace: G' int64, summary u64, parentP, areaP, parentG, areaG int32, inter u32 (all [total]), then the two mark planes (u8)
  char* wsp = reinterpret_cast<char*>(workspace);
  int64_t* gprime = reinterpret_cast<int64_t*>(wsp);
  unsigned long long* summary = reinterpret_cast<unsigned long long*>(wsp + (size_t)total * 8);
  int32_t* parent_p = reinterpret_cast<int32_t*>(wsp + (size_t)total * 16);
  int32_t* area_p = parent_p + total;
  int32_t* parent_g = area_p + total;
  int32_t* area_g = parent_g + total;
  uint32_t* inter = reinterpret_cast<uint32_t*>(area_g + total);
  uint8_t* mark_p = reinterpret_cast<uint8_t*>(wsp + (size_t)total * 36);
  uint8_t* mark_g = mark_p + lm_plane_bytes(total);
  const int conn8 = connectivity == 8;
  const ObjectRule ru = {(long long)min_area, (long long)skip_label, use_skip != 0, K, ignore_index};
  const int rzl = reduce_zero_label ? 1 : 0;
  hipStream_t st = as_stream(s);
  unsigned long long* cnt = reinterpret_cast<unsigned long long*>(counts);

  const int64_t pblocks = cdiv(total, 256 * SV_RUN);
  if (gt_format == SG_GT_I64)
    hipLaunchKernelGGL(object_prepare_kernel<int64_t>, dim3((unsigned)pblocks), dim3(256), 0, st, reinterpret_cast<const int64_t*>(gt), rzl, total, gprime,
                       inter, mark_g);
  else
    hipLaunchKernelGGL(object_prepare_kernel<uint8_t>, dim3((unsigned)pblocks), dim3(256), 0, st, reinterpret_cast<const uint8_t*>(gt), rzl, total, gprime,
                       inter, mark_g);
  SG_LAUNCH_CHECK();
  int64_t wbase = 0;
  for (int n0 = 0; n0 < N;) {                                          // one launch sequence per SG_SIEVE_GROUP images, as sg_sieve
    SieveImages im;
    int64_t tiles = 0, blks = 0;
    n0 += sieve_group(image_hw, offset, N, n0, &wbase, &im, &tiles, &blks);
    const dim3 gp((unsigned)blks);
    SG_TRY(sieve_label(labels, im, tiles, blks, conn8, parent_p, area_p, summary, st));      // zeroes the summaries
    SG_TRY(sieve_label(gprime, im, tiles, blks, conn8, parent_g, area_g, nullptr, st));
    ObjectBlocks ob;                                                   // a sixteenth of the per-pixel workgroups, rounded up per image
    int64_t vblks = 0;
    for (int k = 0; k <= SV_GROUP; ++k) {
      ob.prefix[k] = (int)vblks;
      if (k < im.n) vblks += cdiv((int64_t)im.h[k] * im.w[k], (int64_t)OM_CHUNKS * SV_PIX);
    }
    const dim3 gv((unsigned)vblks);
    hipLaunchKernelGGL(object_vote_kernel<false>, gv, dim3(256), 0, st, labels, (const int64_t*)gprime, im, ob, ru, (const int32_t*)parent_p,
                       (const int32_t*)area_p, (const int32_t*)parent_g, (const int32_t*)area_g, summary, inter);
    SG_LAUNCH_CHECK();
    hipLaunchKernelGGL(object_vote_kernel<true>, gv, dim3(256), 0, st, labels, (const int64_t*)gprime, im, ob, ru, (const int32_t*)parent_p,
                       (const int32_t*)area_p, (const int32_t*)parent_g, (const int32_t*)area_g, summary, inter);
    SG_LAUNCH_CHECK();
    hipLaunchKernelGGL(object_decide_kernel, gp, dim3(256), 0, st, labels, (const int64_t*)gprime, im, ru, (long long)iou_num, (long long)iou_den,
                       (const int32_t*)parent_p, (const int32_t*)area_p, (const int32_t*)parent_g, (const int32_t*)area_g,
                       (const unsigned long long*)summary, (const uint32_t*)inter, mark_p, mark_g, cnt);
    SG_LAUNCH_CHECK();
    if (match_map) {
      hipLaunchKernelGGL(object_map_kernel, gp, dim3(256), 0, st, (const int64_t*)gprime, im, ru, (const int32_t*)parent_p, (const int32_t*)parent_g,
                         (const int32_t*)area_g, (const uint8_t*)mark_p, (const uint8_t*)mark_g, match_map);
      SG_LAUNCH_CHECK();
    }
  }
  return SG_OK;
}
