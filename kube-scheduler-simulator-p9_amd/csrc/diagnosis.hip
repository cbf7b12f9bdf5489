// Unschedulable diagnosis (ksg_filter_histogram / ksg_fit_error, include/ksg.h):
// how many nodes of a kept pod's cycle ended with each (filter code, framework
// status), counted on the device.  Part of the engine's translation unit
// (engine.hip includes it after ranked.hip).
//
//   k_diag_count  one block of 256 threads per tile of kDiagTile nodes.  Every
//                 node's key is its filter code and the framework.Code of that
//                 failure (view_fail: the statement k_view writes fail_code
//                 with).  Lanes of a wave that share a key are counted with one
//                 ballot and popcount (the leader loop of view_body); the
//                 leader adds the wave's count to the block's LDS table
//                 (kDiagLds slots, claimed by compare-and-swap on the key);
//                 after the tile every live LDS slot is flushed once into the
//                 global table (diag_slots slots, the same claim, an integer
//                 atomic add).
//
// Bounded: a probe sequence visits every slot of its table at most once and no
// thread waits on another.  A key that finds the LDS table full goes straight to
// the global table; a key that finds the global table full sets the overflow word
// and is dropped, so the kernel always finishes.  The host clears the table on
// the stream before the launch and copies table and summary through a pinned
// block with one synchronisation.  Counts are integers: the answer does not
// depend on the order in which waves and blocks arrive.  On overflow the caller
// (host.cpp diag_call) counts the kept filter row on the host instead.
#include "../../include/ksg.h"

namespace ksg {

static_assert(kDiagMax == KSG_DIAG_MAX, "the device table holds KSG_DIAG_MAX slots");
constexpr uint32_t kDiagTile = 512;  // nodes per block: two per thread
constexpr uint32_t kDiagLds = 64;    // slots of a block's LDS table (a power of two)
static_assert(kDiagTile % 256 == 0 && (kDiagLds & (kDiagLds - 1)) == 0, "whole rounds of the block; masked probes");

// (code, status) as a table key; never 0, which marks an empty slot
__device__ __host__ __forceinline__ unsigned long long diag_key(uint32_t code, int status) {
  return (1ull << 63) | ((unsigned long long)code << 8) | (uint32_t)(status + 1);
}
__device__ __forceinline__ uint32_t diag_hash(unsigned long long key) {
  return ((uint32_t)(key ^ (key >> 29)) * 2654435761u) >> 16;
}
// cnt nodes of `key` into the global table (slots: a power of two <= kDiagMax)
__device__ __forceinline__ void diag_global(unsigned long long* gkeys, uint32_t* gcnt, uint32_t* over, uint32_t slots,
                                            unsigned long long key, uint32_t cnt) {
  uint32_t h = diag_hash(key) & (slots - 1);
  for (uint32_t probe = 0; probe < slots; ++probe) {
    const unsigned long long cur = atomicCAS(&gkeys[h], 0ull, key);
    if (cur == 0ull || cur == key) {
      atomicAdd(&gcnt[h], cnt);
      return;
    }
    h = (h + 1) & (slots - 1);
  }
  atomicOr(over, 1u);  // full: the host counts the row itself
}
// ... into the block's LDS table, or past it when that is full
__device__ __forceinline__ void diag_block(unsigned long long* lkeys, uint32_t* lcnt, unsigned long long* gkeys,
                                           uint32_t* gcnt, uint32_t* over, uint32_t slots, unsigned long long key,
                                           uint32_t cnt) {
  uint32_t h = diag_hash(key) & (kDiagLds - 1);
  for (uint32_t probe = 0; probe < kDiagLds; ++probe) {
    const unsigned long long cur = atomicCAS(&lkeys[h], 0ull, key);
    if (cur == 0ull || cur == key) {
      atomicAdd(&lcnt[h], cnt);
      return;
    }
    h = (h + 1) & (kDiagLds - 1);
  }
  diag_global(gkeys, gcnt, over, slots, key, cnt);
}

__global__ __launch_bounds__(256) void k_diag_count(DevCluster C, const uint8_t* prog, const uint32_t* filter, ViewDev V,
                                                    uint32_t slots, unsigned long long* gkeys, uint32_t* gcnt,
                                                    uint32_t* over) {
  __shared__ unsigned long long lkeys[kDiagLds];
  __shared__ uint32_t lcnt[kDiagLds];
  for (uint32_t t = threadIdx.x; t < kDiagLds; t += blockDim.x) {
    lkeys[t] = 0ull;
    lcnt[t] = 0;
  }
  __syncthreads();
  const ksg_prog* h = view(prog).h;
  const uint32_t lane = threadIdx.x & 63;
  for (uint32_t round = 0; round < kDiagTile / 256; ++round) {  // (uniform: every wave runs every round)
    const uint32_t n = blockIdx.x * kDiagTile + round * 256 + threadIdx.x;
    bool need = n < C.N;
    const uint32_t code = need ? filter[n] : KSG_FILTER_NOT_EVALUATED;
    int fp, fc;
    const bool failed = view_fail(C, h, V, code, n, fp, fc);
    const int status = failed ? fc : code == KSG_FILTER_PASS ? 0 : -1;
    for (uint64_t m = __ballot(need); m; m = __ballot(need)) {  // one insert per distinct key of the wave
      const int leader = __ffsll((long long)m) - 1;
      const uint32_t c0 = (uint32_t)__builtin_amdgcn_readlane((int)code, leader);
      const int s0 = __builtin_amdgcn_readlane(status, leader);
      const bool same = need && code == c0 && status == s0;
      const uint32_t cnt = (uint32_t)__popcll(__ballot(same));
      if ((int)lane == leader) diag_block(lkeys, lcnt, gkeys, gcnt, over, slots, diag_key(c0, s0), cnt);
      if (same) need = false;
    }
  }
  __syncthreads();
  for (uint32_t t = threadIdx.x; t < kDiagLds; t += blockDim.x)
    if (lkeys[t]) diag_global(gkeys, gcnt, over, slots, lkeys[t], lcnt[t]);
}

namespace {
// the table: the overflow word (and a pad word), the keys, the counts
constexpr size_t kDiagKeysOff = 8;
constexpr size_t diag_cnt_off(uint32_t slots) { return kDiagKeysOff + (size_t)slots * 8; }
constexpr size_t diag_bytes(uint32_t slots) { return diag_cnt_off(slots) + (size_t)slots * 4; }
constexpr size_t kDiagSumOff = (diag_bytes(kDiagMax) + 15) & ~(size_t)15;  // the summary's place in the pinned block

int diag_counts(Engine& eng, uint32_t j, const Engine::ViewCfg& cfg, Engine::DiagCounts& out, std::string& err) {
  Engine::Impl& I = *eng.impl();
  out.entries.clear();
  out.overflow = false;
  if (!kept_pod(I, j)) {
    err = "outputs not kept for this pod";
    return KSG_E_STATE;
  }
  auto run = [&]() -> bool {
    const uint32_t N = I.N, slots = I.diag_slots;
    if (!I.dg_tab.alloc(diag_bytes(kDiagMax), err)) return false;
    if (!I.sq_host.reserve(kDiagSumOff + sizeof(ksg_pod_summary), err)) return false;
    hipStream_t s = I.stream;
    const size_t bytes = diag_bytes(slots);
    HIPCHK(hipMemsetAsync(I.dg_tab.p, 0, bytes, s));
    if (N) {
      ViewDev V{};
      for (int d = 0; d < KSG_MAX_PLUGINS; ++d) {
        V.prof_of_dev[d] = (int8_t)cfg.prof_of_dev[d];
        V.dev_vol[d] = cfg.dev_vol[d] ? 1 : 0;
      }
      for (int p = 0; p < KSG_MAX_PROFILE; ++p) V.kind[p] = (uint8_t)cfg.kind[p];
      V.n_profile = cfg.n_profile;
      const size_t k = j - I.keep_first;
      hipLaunchKernelGGL(k_diag_count, dim3((N + kDiagTile - 1) / kDiagTile), dim3(256), 0, s, I.cluster(),
                         I.progs.p + I.prog_off[j], I.kfilter.p + k * N, V, slots,
                         reinterpret_cast<unsigned long long*>(I.dg_tab.p + kDiagKeysOff),
                         reinterpret_cast<uint32_t*>(I.dg_tab.p + diag_cnt_off(slots)),
                         reinterpret_cast<uint32_t*>(I.dg_tab.p));
      HIPCHK(hipGetLastError());
    }
    HIPCHK(hipMemcpyAsync(I.sq_host.p, I.dg_tab.p, bytes, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(I.sq_host.p + kDiagSumOff, I.sums.p + j, sizeof(ksg_pod_summary), hipMemcpyDeviceToHost, s));
    return stream_sync(I, s, err);
  };
  if (!run()) return KSG_E_DEVICE;
  const uint32_t slots = I.diag_slots;
  std::memcpy(&out.summary, I.sq_host.p + kDiagSumOff, sizeof(out.summary));
  uint32_t over;
  std::memcpy(&over, I.sq_host.p, sizeof(over));
  out.overflow = over != 0;
  if (out.overflow) return KSG_OK;
  const uint8_t* keys = I.sq_host.p + kDiagKeysOff;
  const uint8_t* cnts = I.sq_host.p + diag_cnt_off(slots);
  for (uint32_t t = 0; t < slots; ++t) {
    unsigned long long key;
    uint32_t cnt;
    std::memcpy(&key, keys + (size_t)t * 8, 8);
    std::memcpy(&cnt, cnts + (size_t)t * 4, 4);
    if (!key) continue;
    out.entries.push_back({(uint32_t)(key >> 8), (int32_t)(key & 0xFFu) - 1, cnt});
  }
  return KSG_OK;
}
}  // namespace

}  // namespace ksg

extern "C" int ksg_filter_histogram(ksg_ctx* ctx, uint32_t q, ksg_filter_bucket* out, uint32_t cap, uint32_t* n_out) {
  if (n_out) *n_out = 0;
  const ksg::DiagRequest rq{out, cap, n_out, false, nullptr, 0, nullptr};
  return ksg::diag_call(ctx, q, out && n_out, "filter_histogram", &ksg::diag_counts, rq);
}

extern "C" int ksg_fit_error(ksg_ctx* ctx, uint32_t q, char* buf, size_t cap, size_t* len) {
  if (len) *len = 0;
  const ksg::DiagRequest rq{nullptr, 0, nullptr, true, buf, cap, len};
  return ksg::diag_call(ctx, q, len != nullptr, "fit_error", &ksg::diag_counts, rq);
}
