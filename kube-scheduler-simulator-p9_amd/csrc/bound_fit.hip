// Eviction fit (ksg_bound_fit / ksg_bound_fit_nodes / ksg_node_evictability,
// include/ksg.h): for every bound pod, would its own node admit it again, and how
// many other nodes would -- the headroom pass with the bound pods on the pod
// axis.  Part of the engine's translation unit (engine.hip includes it after
// headroom.hip).
//
//   k_bound_fit<false>  the (node tile x pod tile) grid of snapshot_query.hip
//                 over the bound pods: sq_rows' rows, the gate sq_live.  A pod's
//                 program lies in the victim store (its offset and the pod's own
//                 local node index are wave-uniform reads, like sq_pod's).  The
//                 profile is walked in order, sq_walk<kPmPlaced>, and
//                 NodeResourcesFit is fit_filter, the one body every kernel runs,
//                 over the register source SqLeft.  On the one lane whose node is
//                 the pod's own the source holds free_r + request_r and left + 1:
//                 the rows with the pod taken off them.
//   k_bound_fit<true>   the same body for one pod with a store of the code per node
//                 (ksg_bound_fit_nodes).
//   k_bound_fit_init    presets the structs: {node, KSG_FILTER_NOT_EVALUATED, 0, 0xFFFFFFFF}.
//   k_node_evict  one thread per bound pod over the finished structs, three
//                 atomicAdds into its node's row (ksg_node_evictability).
//
// Accumulation, all integer: sq_first gives the wave's count of passing nodes and
// the lowest of them off one ballot per slot; lane 0 adds / mins them into the
// block's LDS pair of the pod; after the last pod the block issues
// one global atomicAdd and one atomicMin per pod with a passing node.  own_code
// is a plain store by the one lane of the grid whose node is the pod's own.  The
// answer does not depend on the order in which waves and blocks arrive.
//
// Forward progress: snapshot_query.hip's argument; the loops below hold no return.
#include "../../include/ksg.h"

namespace ksg {

using BoundFit = struct ::ksg_bound_fit;  // (the function of the same name hides the struct's)
using NodeEvict = struct ::ksg_node_evict;
static_assert(sizeof(BoundFit) == 16 && offsetof(BoundFit, own_code) == 4 && offsetof(BoundFit, other_nodes) == 8 &&
                  offsetof(BoundFit, first_other) == 12,
              "the kernel accumulates into the struct's own layout");
static_assert(sizeof(NodeEvict) == 16 && offsetof(NodeEvict, stuck) == 4 && offsetof(NodeEvict, drifted) == 8, "");

__global__ __launch_bounds__(256) void k_bound_fit_init(const int32_t* __restrict__ own, uint32_t goff, uint32_t count,
                                                        BoundFit* out) {
  const uint32_t j = blockIdx.x * 256 + threadIdx.x;
  if (j >= count) return;
  const int32_t o = own[j];
  BoundFit b;
  b.node = o < 0 ? -1 : (int32_t)(goff + (uint32_t)o);
  b.own_code = KSG_FILTER_NOT_EVALUATED;
  b.other_nodes = 0;
  b.first_other = (int32_t)0xFFFFFFFFu;
  out[j] = b;
}

// off / own / out: entry 0 is the launch's first bound pod
template <bool PER_NODE>
__global__ __launch_bounds__(256) void k_bound_fit(DevCluster C, DevProfile F, const uint8_t* __restrict__ store,
                                                   const uint64_t* __restrict__ off, const int32_t* __restrict__ own,
                                                   uint32_t count, BoundFit* out, uint32_t* out_codes) {
  __shared__ uint32_t acc[PER_NODE ? 1 : kSqPods][2];  // other_nodes, first_other (global index)
  if (!PER_NODE) {
    if (threadIdx.x < kSqPods) {
      acc[threadIdx.x][0] = 0;
      acc[threadIdx.x][1] = 0xFFFFFFFFu;
    }
    __syncthreads();
  }
  // the block's node rows, once
  const uint32_t base = blockIdx.x * kSqTile + threadIdx.x;
  int64_t fr[kSqNpt][KSG_MAX_RES];
  int32_t left[kSqNpt];
  sq_rows(C, base, fr, left);
#pragma unroll 1
  for (uint32_t pi = 0; pi < kSqPods; ++pi) {
    const uint32_t j = blockIdx.y * kSqPods + pi;
    if (j >= count) break;  // (block-uniform)
    const ProgView V = view(store + off[j]);
    const uint32_t o = (uint32_t)own[j];  // (0xFFFFFFFF: its node is not in the snapshot; no lane holds it)
    const SqPod pod = sq_pod(C, V.h);
    uint32_t code[kSqNpt];
#pragma unroll
    for (uint32_t k = 0; k < kSqNpt; ++k) {
      const uint32_t n = base + k * 256;
      code[k] = KSG_FILTER_NOT_EVALUATED;
      if (sq_live(C, V, n)) {
        const bool home = n == o;  // the rows with the pod itself taken off them
        int64_t f[KSG_MAX_RES];
#pragma unroll
        for (uint32_t r = 0; r < KSG_MAX_RES; ++r) f[r] = fr[k][r] + (home ? pod.req[r] : 0);
        const SqLeft src{f, left[k] + (home ? 1 : 0)};
        code[k] = sq_walk<kPmPlaced>(C, F, V, n, [&] { return fit_filter(src, &pod, (uint32_t)KSG_MAX_RES); });
      }
    }
    if (PER_NODE) {
#pragma unroll
      for (uint32_t k = 0; k < kSqNpt; ++k) {
        const uint32_t n = base + k * 256;
        if (n < C.N) out_codes[n] = code[k];
      }
      continue;
    }
    // the wave's share of pod j, then lane 0 into the block's pair
    SqBallot pass[kSqNpt];
#pragma unroll
    for (uint32_t k = 0; k < kSqNpt; ++k) {
      const uint32_t n = base + k * 256;
      if (n == o) out[j].own_code = code[k];  // (n < C.N: o is a local node; one lane of the grid)
      pass[k] = __ballot(code[k] == KSG_FILTER_PASS && n != o);
    }
    uint32_t n_pass;
    const uint32_t first = sq_first(C.goff + blockIdx.x * kSqTile, pass, &n_pass);
    if (n_pass && lane0()) {
      atomicAdd(&acc[pi][0], n_pass);
      atomicMin(&acc[pi][1], first);
    }
  }
  if (PER_NODE) return;
  __syncthreads();
  // one global atomic per block and non-zero field
  if (threadIdx.x < kSqPods) {
    const uint32_t j = blockIdx.y * kSqPods + threadIdx.x;
    if (j < count && acc[threadIdx.x][0]) {
      atomicAdd(reinterpret_cast<uint32_t*>(&out[j].other_nodes), acc[threadIdx.x][0]);
      atomicMin(reinterpret_cast<uint32_t*>(&out[j].first_other), acc[threadIdx.x][1]);
    }
  }
}

// ev: the local nodes' rows, zeroed
__global__ __launch_bounds__(256) void k_node_evict(const BoundFit* __restrict__ fit, const int32_t* __restrict__ own,
                                                    uint32_t count, uint32_t N, NodeEvict* ev) {
  const uint32_t b = blockIdx.x * 256 + threadIdx.x;
  if (b >= count) return;
  const int32_t o = own[b];
  if (o < 0 || (uint32_t)o >= N) return;
  const BoundFit f = fit[b];
  atomicAdd(&ev[o].pods, 1);
  if (f.other_nodes == 0) atomicAdd(&ev[o].stuck, 1);
  if (f.own_code != KSG_FILTER_PASS) atomicAdd(&ev[o].drifted, 1);
}

namespace {
// Bound pods [first, first + count) against the snapshot as the stream holds it:
// the structs, the one pod's code row or (the range being every bound pod) the
// node rows, through the pinned block, one synchronisation.  Filter codes leave
// with device positions: host.cpp turns them into profile positions.
int bound_fit_run(Engine& eng, uint32_t first, uint32_t count, const int32_t* own, const BoundFitOut& bo,
                  std::string& err) {
  Engine::Impl& I = *eng.impl();
  const uint32_t N = I.N;
  if (!sq_need_fit(I, "bound_fit", err)) return KSG_E_INVALID;
  if ((size_t)first + count > I.vstore_off.size()) {  // (host.cpp ensured the store for this very bound list)
    err = "bound_fit: bound pod outside the victim store";
    return KSG_E_STATE;
  }
  const bool per_node = bo.codes != nullptr, evict = bo.evict != nullptr;
  const size_t fit_bytes = per_node ? 0 : (size_t)count * sizeof(BoundFit);
  const size_t row_bytes = per_node ? (size_t)N * sizeof(uint32_t) : evict ? (size_t)N * sizeof(NodeEvict) : 0;
  const size_t back_bytes = evict || per_node ? row_bytes : fit_bytes;  // what crosses the host link
  if (!back_bytes) return KSG_OK;
  // the launch inputs: every pod's offset into the store, then its own local node
  SqIn in;
  const size_t at_off = in.add<uint64_t>(count), at_own = in.add<int32_t>(count);
  in.stage();
  if (count) {
    std::memcpy(in.host<uint64_t>(at_off), I.vstore_off.data() + first, (size_t)count * sizeof(uint64_t));
    std::memcpy(in.host<int32_t>(at_own), own + first, (size_t)count * sizeof(int32_t));
  }
  auto enqueue = [&](hipStream_t s) -> bool {
    const uint64_t* d_off = in.dev<const uint64_t>(at_off);
    const int32_t* d_own = in.dev<const int32_t>(at_own);
    BoundFit* d_fit = reinterpret_cast<BoundFit*>(I.sq_out.p);
    uint8_t* d_row = I.sq_out.p + fit_bytes;
    if (per_node) {
      hipLaunchKernelGGL(k_bound_fit<true>, dim3((N + kSqTile - 1) / kSqTile), dim3(256), 0, s, I.cluster(), I.F,
                         I.vstore.p, d_off, d_own, 1u, (BoundFit*)nullptr, reinterpret_cast<uint32_t*>(d_row));
      return true;
    }
    if (count)
      hipLaunchKernelGGL(k_bound_fit_init, dim3((count + 255) / 256), dim3(256), 0, s, d_own, I.cluster().goff, count,
                         d_fit);
    sq_chunks(N, count, [&](uint32_t c0, uint32_t cn, dim3 grid) {
      hipLaunchKernelGGL(k_bound_fit<false>, grid, dim3(256), 0, s, I.cluster(), I.F, I.vstore.p, d_off + c0, d_own + c0, cn,
                         d_fit + c0, (uint32_t*)nullptr);
    });
    if (evict) {
      HIPCHK(hipMemsetAsync(d_row, 0, row_bytes, s));
      if (count)
        hipLaunchKernelGGL(k_node_evict, dim3((count + 255) / 256), dim3(256), 0, s, d_fit, d_own, count, N,
                           reinterpret_cast<NodeEvict*>(d_row));
    }
    return true;
  };
  void* dst = per_node ? (void*)bo.codes : evict ? (void*)bo.evict : (void*)bo.fit;
  const size_t back_at = evict || per_node ? fit_bytes : 0;
  return sq_fetch(I, &in, fit_bytes + row_bytes, back_at, back_bytes, dst, enqueue, err) ? KSG_OK : KSG_E_DEVICE;
}
}  // namespace

}  // namespace ksg

extern "C" int ksg_bound_fit(ksg_ctx* ctx, uint32_t first, uint32_t count, struct ksg_bound_fit* out) {
  return ksg::bound_fit_call(ctx, first, count, false, out != nullptr, nullptr, "bound_fit", &ksg::bound_fit_run,
                             ksg::BoundFitOut{out, nullptr, nullptr});
}

extern "C" int ksg_bound_fit_nodes(ksg_ctx* ctx, uint32_t b, uint32_t* codes, uint32_t n) {
  return ksg::bound_fit_call(ctx, b, 1, false, codes != nullptr, &n, "bound_fit_nodes", &ksg::bound_fit_run,
                             ksg::BoundFitOut{nullptr, codes, nullptr});
}

extern "C" int ksg_node_evictability(ksg_ctx* ctx, struct ksg_node_evict* out, uint32_t n) {
  return ksg::bound_fit_call(ctx, 0, 0, true, out != nullptr, &n, "node_evictability", &ksg::bound_fit_run,
                             ksg::BoundFitOut{nullptr, nullptr, out});
}
