// Ranked candidates (ksg_ranked_nodes, include/ksg.h): the K best feasible nodes
// of a kept pod's cycle in the engine's own selection order, selected on the
// device.  Part of the engine's translation unit (engine.hip includes it at its end).
//
//   k_rank_keys   one block per tile of nodes: every node's selection key from
//                 the pod's kept filter row, raw score rows and summary (the
//                 NormalizeScore, weights and pack_key the selection used; 0 for
//                 an infeasible node), then the tile's KSG_RANK_MAX largest keys,
//                 sorted descending, into the partial buffer
//   k_rank_merge  the same select over a key array: one block per `tile` keys of
//                 the level below, launched level by level until one block is left
//
// Plain bounded grids: no flag, no atomic, no persistent loop, so a pod's list is
// the same bytes on every call.  The host copies the K winning keys (<= 512 B) and
// the pod's summary through a pinned block and unpacks node and total.
#include "../../include/ksg.h"

namespace ksg {

static_assert(kRankTile >= 2 * KSG_RANK_MAX, "a tile holds two partial lists: every merge level shrinks");
static_assert((kRankTile & (kRankTile - 1)) == 0, "the sorting network needs a power of two");

// The block's `tile` keys in LDS (a power of two, >= 2 x KSG_RANK_MAX, <= kRankTile)
// sorted descending: a bitonic network, each thread a compare-exchange of
// tile / 2 / blockDim.x pairs per step.  Keys of feasible nodes are distinct
// (they end in the node index), so the order is total; the zeros sink.
__device__ __forceinline__ void rank_sort_desc(uint64_t* keys, uint32_t tile) {
  for (uint32_t k = 2; k <= tile; k <<= 1)
    for (uint32_t j = k >> 1; j > 0; j >>= 1) {
      __syncthreads();
      for (uint32_t t = threadIdx.x; t < tile / 2; t += blockDim.x) {
        const uint32_t i = ((t & ~(j - 1)) << 1) | (t & (j - 1));  // the pair's lower index: bit j clear
        const uint32_t p = i | j;
        const uint64_t a = keys[i], b = keys[p];
        const bool desc = (i & k) == 0;  // (the last stage, k == tile: descending throughout)
        if (desc ? a < b : a > b) {
          keys[i] = b;
          keys[p] = a;
        }
      }
    }
  __syncthreads();
}
__device__ __forceinline__ void rank_put(const uint64_t* keys, uint64_t* out) {
  if (threadIdx.x < KSG_RANK_MAX) out[(size_t)blockIdx.x * KSG_RANK_MAX + threadIdx.x] = keys[threadIdx.x];
}

__global__ __launch_bounds__(256) void k_rank_keys(DevCluster C, DevProfile F, const uint8_t* prog,
                                                   const ksg_pod_summary* sum, const uint32_t* filter,
                                                   const int32_t* score, uint32_t tile, uint64_t* part) {
  __shared__ uint64_t keys[kRankTile];
  const ProgView V = view(prog);
  const ksg_prog* h = V.h;
  const bool scored = sum->feasible > 1;  // a single feasible node: no scoring ran, its score rows are not read
  const uint32_t ipa_flags = sum->ipa_flags;
  const int nf = h->n_tsc_filter, ns = h->n_tsc_score;
  for (uint32_t t = threadIdx.x; t < tile; t += blockDim.x) {
    const uint32_t n = blockIdx.x * tile + t;
    uint64_t key = 0;
    if (n < C.N && filter[n] == KSG_FILTER_PASS) {
      int64_t tot = 0;
      if (scored) {
        const bool pts_keys = ns > 0 && pts_has_keys(C, V, nf, nf + ns, n);
#pragma unroll
        for (int pos = 0; pos < KSG_MAX_PLUGINS; ++pos) {
          if (pos >= F.n) continue;
          bool use;  // false: the plugin's PreScore returned Skip (not scored)
          const int64_t s = normalize_pos(F.plugins[pos], h, score[(size_t)pos * C.N + n], sum->max_score[pos],
                                          sum->min_score[pos], ipa_flags, pts_keys, use);
          if (use) tot += s * F.weight[pos];
        }
      }
      key = pack_key(tot, F.seed, h->queue_idx, C.goff + n);
    }
    keys[t] = key;
  }
  rank_sort_desc(keys, tile);
  rank_put(keys, part);
}

__global__ __launch_bounds__(256) void k_rank_merge(const uint64_t* __restrict__ in, uint32_t n_in, uint32_t tile,
                                                    uint64_t* __restrict__ out) {
  __shared__ uint64_t keys[kRankTile];
  for (uint32_t t = threadIdx.x; t < tile; t += blockDim.x) {
    const uint32_t i = blockIdx.x * tile + t;
    keys[t] = i < n_in ? in[i] : 0;
  }
  rank_sort_desc(keys, tile);
  rank_put(keys, out);
}

namespace {
constexpr size_t kRankKeyBytes = KSG_RANK_MAX * sizeof(uint64_t);

// The k largest keys of kept pod j (descending, zeros after the feasible nodes')
// and its summary, in the pinned block: keys at 0, the summary at kRankKeyBytes.
bool rank_keys(Engine::Impl& I, uint32_t j, uint32_t k, std::string& err) {
  const uint32_t N = I.N, tile = I.rank_tile;
  const uint32_t tiles = (N + tile - 1) / tile;
  // level 0 holds tiles lists, level 1 at most ceil(tiles x KSG_RANK_MAX / tile); later levels fit in turn
  const size_t n_a = (size_t)tiles * KSG_RANK_MAX;
  const size_t n_b = (n_a + tile - 1) / tile * KSG_RANK_MAX;
  if (!I.rk_part.alloc(std::max<size_t>(n_a + n_b, KSG_RANK_MAX), err)) return false;
  if (!I.sq_host.reserve(kRankKeyBytes + sizeof(ksg_pod_summary), err)) return false;
  hipStream_t s = I.stream;
  uint64_t *a = I.rk_part.p, *b = I.rk_part.p + n_a;
  if (tiles) {
    const size_t kk = j - I.keep_first;
    hipLaunchKernelGGL(k_rank_keys, dim3(tiles), dim3(256), 0, s, I.cluster(), I.F, I.progs.p + I.prog_off[j], I.sums.p + j,
                       I.kfilter.p + kk * N, I.kscore.p + kk * N * KSG_MAX_PLUGINS, tile, a);
    for (uint32_t m = tiles; m > 1;) {  // m lists of KSG_RANK_MAX keys -> one list per `tile` keys
      const uint32_t n_in = m * KSG_RANK_MAX, nb = (n_in + tile - 1) / tile;
      hipLaunchKernelGGL(k_rank_merge, dim3(nb), dim3(256), 0, s, a, n_in, tile, b);
      std::swap(a, b);
      m = nb;
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(I.sq_host.p, a, k * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
  }
  HIPCHK(hipMemcpyAsync(I.sq_host.p + kRankKeyBytes, I.sums.p + j, sizeof(ksg_pod_summary), hipMemcpyDeviceToHost, s));
  return stream_sync(I, s, err);
}

struct RankCall {
  uint32_t k;
  ksg_ranked_node* out;
  uint32_t* n_out;
};
int rank_call(Engine& eng, uint32_t j, void* user, std::string& err) {
  Engine::Impl& I = *eng.impl();
  const RankCall& rc = *static_cast<const RankCall*>(user);
  if (!(I.keep_n && j >= I.keep_first && j < I.keep_first + I.keep_n)) {
    err = "outputs not kept for this pod";
    return KSG_E_STATE;
  }
  if (!rank_keys(I, j, rc.k, err)) return KSG_E_DEVICE;
  ksg_pod_summary sum;
  std::memcpy(&sum, I.sq_host.p + kRankKeyBytes, sizeof(sum));
  if (sum.status != 0 || sum.feasible <= 0 || !I.N) return KSG_OK;  // unschedulable, or the cycle ended in an error
  if (sum.feasible == 1) {  // upstream's shortcut: no scoring, the summary holds the node and its total
    rc.out[0].node = sum.selected;
    rc.out[0].total = (int32_t)(sum.best_key >> 40);
    *rc.n_out = 1;
    return KSG_OK;
  }
  const uint32_t n = std::min<uint32_t>(rc.k, (uint32_t)sum.feasible);
  const uint64_t* keys = reinterpret_cast<const uint64_t*>(I.sq_host.p);
  for (uint32_t i = 0; i < n; ++i) {
    if (!keys[i]) {
      err = "ranked_nodes: the pod's kept outputs hold fewer feasible nodes than its summary";
      return KSG_E_STATE;
    }
    rc.out[i].node = (int32_t)(keys[i] & 0xFFFFFull);
    rc.out[i].total = (int32_t)(keys[i] >> 40);
  }
  *rc.n_out = n;
  return KSG_OK;
}
}  // namespace

}  // namespace ksg

extern "C" int ksg_ranked_nodes(ksg_ctx* ctx, uint32_t q, uint32_t k, ksg_ranked_node* out, uint32_t* n_out) {
  if (n_out) *n_out = 0;
  ksg::RankCall rc{k, out, n_out};
  const bool args_ok = k >= 1 && k <= KSG_RANK_MAX && out && n_out;
  return ksg::kept_pod_call(ctx, q, args_ok, "ranked_nodes", &ksg::rank_call, &rc);
}
