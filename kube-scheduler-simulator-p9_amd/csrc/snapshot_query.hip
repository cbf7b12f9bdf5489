// Snapshot queries: what the entry points that ask the device snapshot a question
// and return the answer in one synchronisation share (ranked.hip, diagnosis.hip,
// headroom.hip, bound_fit.hip, drain.hip, scale_up.hip; DESIGN.md "Snapshot
// queries").  Part of the engine's translation unit (engine.hip includes it
// before ranked.hip).
//
// Device, for the last four: a block of 256 threads holds kSqTile rows in
// registers, kSqNpt a thread, as what is left of them, and judges pods against
// them one after another; a pod's header and requests are wave-uniform reads
// through the scalar cache.  Every helper is __forceinline__ and takes the row
// arrays by reference: a slot is selected by an unrolled predicated loop, never
// by a run-time register index, which would put the rows into scratch.  The pod
// loop stays in each kernel: three lines, whose `continue`s would read `return`.
//
// Forward progress: no thread waits on another thread's progress.  The only
// waits are block barriers (SqFirstHit::step is one), which every thread of a
// block reaches: the loops hold no return and their breaks are block-uniform.
// Every loop is bounded by a tile constant, the profile length or KSG_MAX_RES.
#include <cassert>

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

// A placed or placeable pod's static filters (its spec.nodeName is its placement); headroom adds NodeName
constexpr uint32_t kPmPlaced = (1u << KP_TAINT) | (1u << KP_NA) | (1u << KP_UNSCHED);
constexpr uint32_t kPmHeadroom = kPmPlaced | (1u << KP_NODENAME);

// fit_filter's pod: the flags and the requests on the cluster's columns (0 beyond them)
struct SqPod {
  uint32_t flags;
  int64_t req[KSG_MAX_RES];
};
__device__ __forceinline__ SqPod sq_pod(const DevCluster& C, const ksg_prog* h) {
  SqPod pod;
  pod.flags = h->flags;
#pragma unroll
  for (uint32_t r = 0; r < KSG_MAX_RES; ++r) pod.req[r] = r < C.R ? h->req[r] : 0;
  return pod;
}
// fit_filter's operand source over a row held in registers, as what is left of it
struct SqLeft {
  const int64_t (&fr)[KSG_MAX_RES];
  int32_t left;
  __device__ __forceinline__ int64_t allocatable(int res) const { return fr[res]; }
  __device__ __forceinline__ int64_t requested(int) const { return 0; }
  __device__ __forceinline__ int32_t podcnt() const { return 0; }
  __device__ __forceinline__ int32_t allowed() const { return left; }
};

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

// The wave's lowest passing index, 0xFFFFFFFF if none, wave-uniform; n_pass, if given: how many pass.
// pass[k]: the wave's ballot of slot k's predicate, taken where the predicate is computed (kept as a
// bool per lane across the slots it costs a register round trip); thread t's slot k holds index
// base + k x 256 + t (base: block-uniform).  The lowest is "the lowest k with a set bit, then its
// lowest lane": exact only because a lane's indices ascend with k and the wave's 64 lanes are
// contiguous within a slot.
using SqBallot = unsigned long long;
__device__ __forceinline__ uint32_t sq_first(uint32_t base, const SqBallot (&pass)[kSqNpt], uint32_t* n_pass = nullptr) {
  uint32_t first = 0xFFFFFFFFu, n = 0;
#pragma unroll
  for (uint32_t k = 0; k < kSqNpt; ++k) {
    const SqBallot b = pass[k];
    if (!b) continue;  // (wave-uniform)
    n += (uint32_t)__popcll(b);
    if (first == 0xFFFFFFFFu) first = base + k * 256 + (threadIdx.x & ~63u) + (uint32_t)__ffsll((long long)b) - 1;
  }
  if (n_pass) *n_pass = n;
  return first;
}

// The block's lowest hit of one step after another, through three LDS words used in rotation: step
// number `it` uses word it % 3.  The waves min into it before the step's barrier, every thread reads it
// after the barrier, and thread 0 then presets word (it + 2) % 3.  One barrier per step is enough: that
// word was last read in step it - 1, by threads that have since arrived at this barrier, and is next
// written in step it + 2, by threads that have passed the barrier of step it + 1, which thread 0
// reaches only after the preset.  (With two words the preset and the next step's mins would meet with
// no barrier between them.)  step is a block barrier: all threads of the block call it, or none.
struct SqFirstHit {
  uint32_t (&hit)[3];  // __shared__ in the kernel
  uint32_t it;
  __device__ __forceinline__ void init() {  // (the barrier also publishes what thread 0 stored before the call)
    if (threadIdx.x == 0) hit[0] = hit[1] = hit[2] = 0xFFFFFFFFu;
    it = 0;
    __syncthreads();
  }
  __device__ __forceinline__ uint32_t step(uint32_t first) {  // first: sq_first's; returns the block's, block-uniform
    if (first != 0xFFFFFFFFu && lane0()) atomicMin(&hit[it % 3], first);
    __syncthreads();
    const uint32_t found = hit[it % 3];
    if (threadIdx.x == 0) hit[(it + 2) % 3] = 0xFFFFFFFFu;
    ++it;
    return found;
  }
};

namespace {
// Host.  Every run function's first refusal (host.cpp checked the profile; the kernels read a Fit profile)
bool sq_need_fit(const Engine::Impl& I, const char* what, std::string& err) {
  if (I.F.n && I.F.pos_fit >= 0) return true;
  err = std::string(what) + ": NodeResourcesFit is not in the profile";
  return false;
}

// A call's launch inputs, one staging buffer uploaded to I.sq_in in one copy.  Two phases: add<T>(n) lays
// the typed arrays out one after another, each at an 8-byte boundary, and returns their offsets; stage()
// allocates once; host<T> / dev<T> then give an array at its offset on either side.
struct SqIn {
  std::vector<uint8_t> bytes;
  size_t size = 0, device_only = 0;  // bytes of the inputs; bytes reserved behind them on the device, not uploaded
  uint8_t* d = nullptr;              // I.sq_in.p, once sq_fetch has allocated it
  size_t end() const { return (size + 7) & ~(size_t)7; }
  template <class T>
  size_t add(size_t n) {
    assert(bytes.empty() && !device_only);
    const size_t at = end();
    size = at + n * sizeof(T);
    return at;
  }
  // n bytes that the kernels write and read; the last thing added (add asserts that none follows); returns their offset
  size_t reserve(size_t n) { return device_only = n, end(); }
  void stage() { bytes.resize(size); }
  template <class T>
  T* host(size_t at) { return reinterpret_cast<T*>(bytes.data() + at); }
  template <class T>
  T* dev(size_t at) const { return reinterpret_cast<T*>(d + at); }
};

// A call's round trip: `in` (if any) uploaded to I.sq_in, out_bytes of I.sq_out for the kernels, the
// caller's enqueue on the engine stream (false: err is set), back_bytes from offset back_at of I.sq_out
// through the pinned block, one synchronisation: the answer is then at I.sq_host.p, and at dst if that
// is given.  false: a device error, err is set.
template <class Enqueue>
bool sq_fetch(Engine::Impl& I, SqIn* in, size_t out_bytes, size_t back_at, size_t back_bytes, void* dst, Enqueue enqueue,
              std::string& err) {
  if (in && !I.sq_in.alloc(in->end() + in->device_only, err)) return false;
  if (!I.sq_out.alloc(out_bytes, err) || !I.sq_host.reserve(back_bytes, err)) return false;
  hipStream_t s = I.stream;
  if (in) in->d = I.sq_in.p;
  if (in && in->size) HIPCHK(hipMemcpyAsync(in->d, in->bytes.data(), in->size, hipMemcpyHostToDevice, s));
  if (!enqueue(s)) return false;
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(I.sq_host.p, I.sq_out.p + back_at, back_bytes, hipMemcpyDeviceToHost, s));
  if (!stream_sync(I, s, err)) return false;
  if (dst) std::memcpy(dst, I.sq_host.p, back_bytes);
  return true;
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
