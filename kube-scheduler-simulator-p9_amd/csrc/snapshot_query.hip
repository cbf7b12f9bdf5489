// Snapshot queries: what the entry points that ask the device snapshot a question
// and return the answer in one synchronisation share (ranked.hip, diagnosis.hip,
// headroom.hip, bound_fit.hip; DESIGN.md "Snapshot queries").  Part of the
// engine's translation unit (engine.hip includes it before ranked.hip).
//
// Device, for k_headroom and k_bound_fit: a block of 256 threads owns kSqTile
// nodes, loads their rows once into registers (sq_rows) and walks the kSqPods pods
// of its pod tile over them; a pod's header and requests are wave-uniform reads
// through the scalar cache.  The pod loop stays in each kernel: it is three
// lines, and as a callable its `continue`s would read `return`.
//
// Forward progress: no thread waits on another thread's progress.  The only
// waits are block barriers, which every thread of a block reaches: the pod and
// node loops hold no return, and the pod loop's `j >= count` break is
// block-uniform.  Every loop is bounded by a tile constant, the profile length
// or KSG_MAX_RES.
namespace ksg {

// (several node blocks per pod from 1025 nodes, several pod tiles from 33 pods: no override is read)
constexpr uint32_t kSqNpt = 4;                        // nodes per thread
constexpr uint32_t kSqTile = 256 * kSqNpt;            // nodes per block
constexpr uint32_t kSqPods = 32;                      // pods per block (grid.y tiles)
constexpr uint32_t kSqLaunchPods = 65535u * kSqPods;  // pods one launch covers at most (grid.y <= 65535)

// The rows of the thread's nodes base + k x 256, as what is left of them: free_r = allocatable_r -
// requested_r for the R resource columns, left = allowed - pod count (0 beyond columns and snapshot)
__device__ __forceinline__ void sq_rows(const DevCluster& C, uint32_t base, int64_t (&fr)[kSqNpt][KSG_MAX_RES],
                                        int32_t (&left)[kSqNpt]) {
#pragma unroll
  for (uint32_t k = 0; k < kSqNpt; ++k) {
    const uint32_t n = base + k * 256;
    const bool live = n < C.N;
    left[k] = live ? C.allowed[n] - C.podcnt[n] : 0;
#pragma unroll
    for (uint32_t r = 0; r < KSG_MAX_RES; ++r)
      fr[k][r] = (live && r < C.R) ? C.alloc[(size_t)r * C.N + n] - C.req[(size_t)r * C.N + n] : 0;
  }
}

// Node n is live for the pod of V: in the snapshot, the pod's PreFilter neither rejected nor failed, n in
// its PreFilterResult bitmask if it has one (as k_eval reads them; k_whatif's gate differs on purpose)
__device__ __forceinline__ bool sq_live(const DevCluster& C, const ProgView& V, uint32_t n) {
  const ksg_prog* h = V.h;
  const uint32_t flags = h->flags;
  return n < C.N && !(flags & (KPF_PREFILTER_REJECT | KPF_PREFILTER_ERROR)) &&
         !((flags & KPF_RESTRICT) && !bit(V.u32 + h->restrict_off, h->restrict_words, (int32_t)n));
}

// The profile in order on node n until a filter fails: node_filter<PM>, the switch every kernel shares,
// and at NodeResourcesFit's position the caller's fit(), which returns fit_filter's reason bits.
// Without fit, Fit is no part of the walk (it is outside PM, where node_filter passes).
struct SqNoFit {
  __device__ uint32_t operator()() const { return 0; }
};
template <uint32_t PM, class Fit = SqNoFit>
__device__ __forceinline__ uint32_t sq_walk(const DevCluster& C, const DevProfile& F, const ProgView& V, uint32_t n,
                                            Fit fit = Fit{}) {
  uint32_t code = KSG_FILTER_PASS;
#pragma unroll 1
  for (int pos = 0; pos < F.n && code == KSG_FILTER_PASS; ++pos) {
    const int plugin = F.plugins[pos];
    if (std::is_same<Fit, SqNoFit>::value || plugin != KP_FIT) code = node_filter<PM>(plugin, pos, C, V, n);
    else if (const uint32_t detail = fit()) code = filter_code(pos, detail);
  }
  return code;
}

namespace {
// Host.  Reserve the pinned block, run the caller's enqueue on the engine stream (false: err is set),
// copy `bytes` back from device address src, synchronise once: the answer is then at I.sq_host.p.
template <class Enqueue>
bool sq_fetch(Engine::Impl& I, const void* src, size_t bytes, Enqueue enqueue, std::string& err) {
  if (!I.sq_host.reserve(bytes, err)) return false;
  hipStream_t s = I.stream;
  if (!enqueue(s)) return false;
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(I.sq_host.p, src, bytes, hipMemcpyDeviceToHost, s));
  return stream_sync(I, s, err);
}

// launch(c0, cn, grid) for every chunk [c0, c0 + cn) of `count` pods that one
// (node tile x pod tile) grid covers; nothing on an empty snapshot
template <class Launch>
void sq_chunks(uint32_t N, uint32_t count, Launch launch) {
  const uint32_t tiles = (N + kSqTile - 1) / kSqTile;
  for (uint32_t c0 = 0; tiles && c0 < count; c0 += kSqLaunchPods) {
    const uint32_t cn = std::min(count - c0, kSqLaunchPods);
    launch(c0, cn, dim3(tiles, (cn + kSqPods - 1) / kSqPods));
  }
}
}  // namespace

}  // namespace ksg
