// Headroom (ksg_headroom / ksg_headroom_nodes, include/ksg.h): how many more
// copies of a queue pod fit on every node of the device snapshot, counted on the
// device.  Part of the engine's translation unit (engine.hip includes it after
// diagnosis.hip).
//
//   k_headroom<false>  the (node tile x pod tile) grid of snapshot_query.hip
//                 over the queue pods: the rows are sq_rows' with room = max(0,
//                 left), the gate is sq_live, the static filters are
//                 sq_walk<kPmHeadroom> (their per-node operands -- taints,
//                 labels, the node flags -- are read there, from L1/L2 after the
//                 tile's first pod).  The count is a running minimum:
//                 it starts at the room and every requested column r lowers it to
//                 div_cap(free_r, req_r, count), so the constraint that lowered it
//                 last is the lowest index holding the minimum (bound[]).
//   k_headroom<true>   the same body for one pod with a store per node instead of
//                 the reduction (ksg_headroom_nodes).
//
// Accumulation, all integer: per wave the node counts and bound[] are ballots
// and popcounts, the replica sum and the (count, node) key DPP reductions of
// 32-bit words (the form of wave_max_u64; no 64-bit shuffle); lane 0 adds the
// wave's values to the block's LDS copy of the pod tile's result structs; after
// the last pod the block adds every non-zero LDS word to the device structs,
// one global atomic per block and field.  max_node / best_node travel as one
// 64-bit key, (count << 32) | (0xFFFFFFFF - global node), under an atomic max
// in the place of the two fields; the host decodes it.  The answer does not
// depend on the order in which waves and blocks arrive.
//
// Forward progress: snapshot_query.hip's argument; the loops below hold no return.
#include "../../include/ksg.h"

namespace ksg {

using Headroom = struct ::ksg_headroom;  // (the function of the same name hides the struct's)
constexpr uint32_t kHrWords = sizeof(Headroom) / 4;
static_assert(KSG_HEADROOM_BOUNDS == 1 + KSG_MAX_RES, "bound[]: the pod room, then every resource column");
static_assert(sizeof(Headroom) == 64 && offsetof(Headroom, nodes) == 8 && offsetof(Headroom, open_nodes) == 12 &&
                  offsetof(Headroom, max_node) == 16 && offsetof(Headroom, best_node) == 20 &&
                  offsetof(Headroom, bound) == 24,
              "the kernel accumulates into the struct's own layout; the key lies over max_node / best_node");
// 32-bit words of a struct ksg_headroom
enum : uint32_t { kHrwReplicas = 0, kHrwNodes = 2, kHrwOpen = 3, kHrwKey = 4, kHrwBound = 6 };

// The sum of a non-negative 64-bit value below 2^40 over the wave's active lanes,
// as two 32-bit DPP sums (64 x 2^20 fits either; wave_max_u64's note on 64-bit shuffles)
__device__ __forceinline__ uint64_t wave_sum_u40(uint64_t v) {
  const uint32_t lo = (uint32_t)__ockl_wfred_add_i32((int32_t)(v & 0xFFFFFu));
  const uint32_t hi = (uint32_t)__ockl_wfred_add_i32((int32_t)(v >> 20));
  return ((uint64_t)hi << 20) + lo;
}

template <bool PER_NODE>
__global__ __launch_bounds__(256) void k_headroom(DevCluster C, DevProfile F, const uint8_t* __restrict__ progs,
                                                  const uint64_t* __restrict__ prog_off, uint32_t q0, uint32_t count,
                                                  Headroom* out, int32_t* out_nodes) {
  __shared__ __attribute__((aligned(16))) uint32_t acc[PER_NODE ? 1 : kSqPods * kHrWords];  // (64-bit words inside)
  if (!PER_NODE) {
    for (uint32_t t = threadIdx.x; t < kSqPods * kHrWords; t += 256) acc[t] = 0;
    __syncthreads();
  }
  // the block's node rows, once
  const uint32_t base = blockIdx.x * kSqTile + threadIdx.x;
  int64_t fr[kSqNpt][KSG_MAX_RES];
  int32_t room[kSqNpt];
  sq_rows(C, base, fr, room);
#pragma unroll
  for (uint32_t k = 0; k < kSqNpt; ++k) room[k] = room[k] > 0 ? room[k] : 0;
#pragma unroll 1
  for (uint32_t pi = 0; pi < kSqPods; ++pi) {
    const uint32_t j = blockIdx.y * kSqPods + pi;
    if (j >= count) break;  // (block-uniform)
    const ProgView V = view(progs + prog_off[q0 + j]);
    const ksg_prog* h = V.h;
    const uint32_t flags = h->flags;
    bool open[kSqNpt];
    int32_t cnt[kSqNpt];
    uint32_t which[kSqNpt];
#pragma unroll
    for (uint32_t k = 0; k < kSqNpt; ++k) {
      const uint32_t n = base + k * 256;
      const bool ok = sq_live(C, V, n) && sq_walk<kPmHeadroom>(C, F, V, n) == KSG_FILTER_PASS;
      open[k] = ok;
      cnt[k] = ok ? room[k] : 0;
      which[k] = 0;
    }
    if (!(flags & KPF_ZERO_REQUEST)) {  // (fit_filter: no resource is looked at for a zero-request pod)
#pragma unroll
      for (uint32_t r = 0; r < KSG_MAX_RES; ++r) {
        const int64_t rq = h->req[r];
        if (r >= C.R || rq <= 0) continue;  // (wave-uniform)
#pragma unroll
        for (uint32_t k = 0; k < kSqNpt; ++k) {
          if (!open[k]) continue;
          const int64_t f = fr[k][r];
          const int32_t fit = f < 0 ? 0 : (int32_t)div_cap(f, rq, cnt[k]);
          if (fit < cnt[k]) {  // (a tie keeps the lower index)
            cnt[k] = fit;
            which[k] = 1 + r;
          }
        }
      }
    }
    if (PER_NODE) {
#pragma unroll
      for (uint32_t k = 0; k < kSqNpt; ++k) {
        const uint32_t n = base + k * 256;
        if (n < C.N) out_nodes[n] = cnt[k];
      }
      continue;
    }
    // the wave's share of pod j, then lane 0 into the block's struct
    uint64_t sum = 0, key = 0;
    uint32_t n_pos = 0, n_open = 0;
#pragma unroll
    for (uint32_t k = 0; k < kSqNpt; ++k) {
      sum += (uint32_t)cnt[k];
      const uint64_t kk = ((uint64_t)(uint32_t)cnt[k] << 32) | (0xFFFFFFFFu - (C.goff + base + k * 256));
      if (cnt[k] > 0 && kk > key) key = kk;
      n_pos += (uint32_t)__popcll(__ballot(cnt[k] > 0));
      n_open += (uint32_t)__popcll(__ballot(open[k]));
    }
    if (n_open == 0) continue;  // (wave-uniform: nothing of this wave counts for the pod)
    const uint64_t wsum = wave_sum_u40(sum);
    const uint64_t wkey = wave_max_u64(key);
    uint32_t* a = acc + pi * kHrWords;
    if (lane0()) {
      atomicAdd(a + kHrwOpen, n_open);
      if (n_pos) {
        atomicAdd(reinterpret_cast<unsigned long long*>(a + kHrwReplicas), (unsigned long long)wsum);
        atomicAdd(a + kHrwNodes, n_pos);
        atomicMax(reinterpret_cast<unsigned long long*>(a + kHrwKey), (unsigned long long)wkey);
      }
    }
    for (uint32_t i = 0; i < 1 + C.R; ++i) {  // (R <= KSG_MAX_RES: the columns the cluster has)
      uint32_t c = 0;
#pragma unroll
      for (uint32_t k = 0; k < kSqNpt; ++k) c += (uint32_t)__popcll(__ballot(open[k] && which[k] == i));
      if (c && lane0()) atomicAdd(a + kHrwBound + i, c);
    }
  }
  if (PER_NODE) return;
  __syncthreads();
  // one global atomic per block and non-zero field
  const uint32_t pods = count - blockIdx.y * kSqPods < kSqPods ? count - blockIdx.y * kSqPods : kSqPods;
  for (uint32_t t = threadIdx.x; t < pods * kHrWords; t += 256) {
    const uint32_t pi = t / kHrWords, w = t % kHrWords;
    uint32_t* g = reinterpret_cast<uint32_t*>(out + (size_t)blockIdx.y * kSqPods + pi) + w;
    const uint32_t* a = acc + pi * kHrWords + w;
    if (w == kHrwReplicas || w == kHrwKey) {
      const unsigned long long v = *reinterpret_cast<const unsigned long long*>(a);
      if (!v) continue;
      if (w == kHrwReplicas) atomicAdd(reinterpret_cast<unsigned long long*>(g), v);
      else atomicMax(reinterpret_cast<unsigned long long*>(g), v);
    } else if (w == kHrwNodes || w == kHrwOpen || (w >= kHrwBound && w < kHrwBound + KSG_HEADROOM_BOUNDS)) {
      if (*a) atomicAdd(g, *a);
    }
  }
}

namespace {
struct HeadroomCall {
  Headroom* out;       // ksg_headroom: count structs
  int32_t* out_nodes;  // ksg_headroom_nodes: N counts of pod `first`
};
// Queue pods [first, first + count) against the snapshot as the stream holds it:
// the structs (or the one pod's node row) through the pinned block, one synchronisation
int headroom_run(Engine& eng, uint32_t first, uint32_t count, void* user, std::string& err) {
  Engine::Impl& I = *eng.impl();
  const HeadroomCall& hc = *static_cast<const HeadroomCall*>(user);
  const bool per_node = hc.out_nodes != nullptr;
  const uint32_t N = I.N;
  if (!sq_need_fit(I, "headroom", err)) return KSG_E_INVALID;
  const size_t bytes = per_node ? (size_t)N * sizeof(int32_t) : (size_t)count * sizeof(Headroom);
  if (!bytes) return KSG_OK;
  auto enqueue = [&](hipStream_t s) -> bool {
    if (per_node) {
      hipLaunchKernelGGL(k_headroom<true>, dim3((N + kSqTile - 1) / kSqTile), dim3(256), 0, s, I.cluster(), I.F, I.progs.p,
                         I.prog_off_d.p, first, 1u, (Headroom*)nullptr, reinterpret_cast<int32_t*>(I.sq_out.p));
      return true;
    }
    HIPCHK(hipMemsetAsync(I.sq_out.p, 0, bytes, s));
    sq_chunks(N, count, [&](uint32_t c0, uint32_t cn, dim3 grid) {
      hipLaunchKernelGGL(k_headroom<false>, grid, dim3(256), 0, s, I.cluster(), I.F, I.progs.p, I.prog_off_d.p, first + c0,
                         cn, reinterpret_cast<Headroom*>(I.sq_out.p) + c0, (int32_t*)nullptr);
    });
    return true;
  };
  if (!sq_fetch(I, nullptr, bytes, 0, bytes, hc.out_nodes, enqueue, err)) return KSG_E_DEVICE;
  if (per_node) return KSG_OK;
  for (uint32_t i = 0; i < count; ++i) {  // the key back into its two fields
    Headroom hr;
    std::memcpy(&hr, I.sq_host.p + (size_t)i * sizeof(hr), sizeof(hr));
    uint64_t key;
    std::memcpy(&key, reinterpret_cast<const uint8_t*>(&hr) + kHrwKey * 4, sizeof(key));
    hr.max_node = (int32_t)(key >> 32);
    hr.best_node = key ? (int32_t)(0xFFFFFFFFu - (uint32_t)key) : -1;
    hc.out[i] = hr;
  }
  return KSG_OK;
}
}  // namespace

}  // namespace ksg

extern "C" int ksg_headroom(ksg_ctx* ctx, uint32_t first, uint32_t count, struct ksg_headroom* out) {
  ksg::HeadroomCall hc{out, nullptr};
  return ksg::headroom_call(ctx, first, count, out != nullptr, nullptr, "headroom", &ksg::headroom_run, &hc);
}

extern "C" int ksg_headroom_nodes(ksg_ctx* ctx, uint32_t q, int32_t* out, uint32_t n) {
  ksg::HeadroomCall hc{nullptr, out};
  return ksg::headroom_call(ctx, q, 1, out != nullptr, &n, "headroom_nodes", &ksg::headroom_run, &hc);
}
