// Scale-up simulation (ksg_scale_up / ksg_scale_up_plan, include/ksg.h): pack a
// list of queue pods onto fresh nodes of a template's shape, first fit in bin
// order, once per template.  Part of the engine's translation unit (engine.hip
// includes it after drain.hip).
//
//   k_scale_open   the (pods x templates) grid, one thread per pair, fully
//                 parallel: open(p, t) -- the pod's PreFilter neither rejected
//                 nor failed, it has no PreFilterResult node set, with NodeName
//                 in the profile it names no node, and sq_walk<kPmPlaced> passes
//                 on node t -- stored as one byte per pair, row t of n_pods bytes.
//   k_scale_pack<false>  one block of 256 threads per template.  Bin j lives in
//                 the registers of thread j % 256, slot j / 256: kSqTile bins, as
//                 what is left of them (sq_rows' form), every bin initialised to
//                 the empty fresh node: allocatable_r(t) - base_r and allowed(t) -
//                 base_pods.  For each pod in list order: a closed pod (its byte)
//                 is counted and skipped by the whole block; otherwise every lane
//                 tests its bins with index <= min(nodes, cap - 1) with fit_filter
//                 (bin `nodes` is the next fresh node, still empty), and the
//                 block's lowest admitting bin is sq_first's through
//                 SqFirstHit::step, one barrier per open pod.  The owning lane
//                 lowers its bin; a hit at index == nodes opens that bin.  Every
//                 thread keeps `nodes` and the counts in registers (they are
//                 block-uniform).  No hit with nodes < cap: the empty node itself
//                 did not admit the pod (too big); with nodes == cap the empty
//                 node is tested apart, uniformly (too big or over the cap).  At
//                 the end thread 0 stores the 32-byte struct.
//   k_scale_pack<true>   the same body for one template with a store of the bin
//                 per listed pod (ksg_scale_up_plan).
//
// The base load is summed on the host (host.cpp scale_up_call) and arrives with
// the launch inputs; the kernels read the queue's programs and the node columns
// and write nothing but the open bytes and the answer.
//
// Forward progress: snapshot_query.hip's argument.  The pod loop's bound is a
// kernel argument, and the skip of a closed pod reads one byte at a block-uniform
// address, so the barrier of an open pod is reached by all threads or none.
#include "../../include/ksg.h"

namespace ksg {

using ScaleUp = struct ::ksg_scale_up;  // (the function of the same name hides the struct's)
static_assert(KSG_SCALE_MAX == kScaleMax && kScaleMax == kSqTile, "the header's cap is the bins one block holds");
static_assert(sizeof(ScaleUp) == 32 && offsetof(ScaleUp, packed) == 4 && offsetof(ScaleUp, over_cap) == 16 &&
                  offsetof(ScaleUp, first_unpacked) == 20 && offsetof(ScaleUp, base_pods) == 24 &&
                  offsetof(ScaleUp, reserved) == 28,
              "the kernel stores the struct's own layout");
// one template's launch input: what every fresh node of it starts with
struct ScaleBase {
  int64_t req[KSG_MAX_RES];
  int32_t pods, pad;
};
constexpr int32_t kScaleClosed = -1, kScaleTooBig = -2, kScaleOverCap = -3;  // the plan's codes

// pods: the list (queue indices); tmpl: entry 0 is the launch's first template; open: its row
__global__ __launch_bounds__(256) void k_scale_open(DevCluster C, DevProfile F, const uint8_t* __restrict__ progs,
                                                    const uint64_t* __restrict__ prog_off,
                                                    const uint32_t* __restrict__ pods, uint32_t n_pods,
                                                    const uint32_t* __restrict__ tmpl, uint32_t has_nodename,
                                                    uint8_t* open) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n_pods) return;
  const uint32_t t = tmpl[blockIdx.y];
  const ProgView V = view(progs + prog_off[pods[i]]);
  const ksg_prog* h = V.h;
  const uint32_t flags = h->flags;
  const bool ok = t < C.N && !(flags & (KPF_PREFILTER_REJECT | KPF_PREFILTER_ERROR | KPF_RESTRICT)) &&
                  !(has_nodename && h->node_name_gid != -1) && sq_walk<kPmPlaced>(C, F, V, t) == KSG_FILTER_PASS;
  open[(size_t)blockIdx.y * n_pods + i] = ok ? 1 : 0;
}

// cap: max_nodes, in [1, kScaleMax]
template <bool PLAN>
__global__ __launch_bounds__(256) void k_scale_pack(DevCluster C, const uint8_t* __restrict__ progs,
                                                    const uint64_t* __restrict__ prog_off,
                                                    const uint32_t* __restrict__ pods, uint32_t n_pods,
                                                    const uint32_t* __restrict__ tmpl,
                                                    const ScaleBase* __restrict__ base,
                                                    const uint8_t* __restrict__ open, uint32_t cap, ScaleUp* out,
                                                    int32_t* plan) {
  __shared__ uint32_t hit[3];
  const uint32_t tid = threadIdx.x;
  SqFirstHit bin_hit{hit};
  bin_hit.init();
  const uint32_t t = tmpl[blockIdx.x];
  const uint8_t* row = open + (size_t)blockIdx.x * n_pods;
  // the empty fresh node, then every bin as a copy of it
  int64_t e_fr[KSG_MAX_RES];
  const int32_t base_pods = base[blockIdx.x].pods;
  const int32_t e_left = t < C.N ? C.allowed[t] - base_pods : 0;
#pragma unroll
  for (uint32_t r = 0; r < KSG_MAX_RES; ++r)
    e_fr[r] = (t < C.N && r < C.R) ? C.alloc[(size_t)r * C.N + t] - base[blockIdx.x].req[r] : 0;
  int64_t fr[kSqNpt][KSG_MAX_RES];
  int32_t left[kSqNpt];
#pragma unroll
  for (uint32_t k = 0; k < kSqNpt; ++k) {
    left[k] = e_left;
#pragma unroll
    for (uint32_t r = 0; r < KSG_MAX_RES; ++r) fr[k][r] = e_fr[r];
  }
  uint32_t nodes = 0;
  int32_t packed = 0, closed = 0, too_big = 0, over_cap = 0, first_unpacked = -1;  // (block-uniform)
#pragma unroll 1
  for (uint32_t i = 0; i < n_pods; ++i) {
    int32_t bin;
    if (!row[i]) {  // (block-uniform)
      ++closed;
      bin = kScaleClosed;
    } else {
      const SqPod pod = sq_pod(C, view(progs + prog_off[pods[i]]).h);
      const uint32_t last = nodes < cap ? nodes : cap - 1;  // the highest bin tested: the next fresh node, or the cap's last
      SqBallot pass[kSqNpt];
#pragma unroll
      for (uint32_t k = 0; k < kSqNpt; ++k)
        pass[k] = __ballot(k * 256 + tid <= last && fit_filter(SqLeft{fr[k], left[k]}, &pod, (uint32_t)KSG_MAX_RES) == 0);
      const uint32_t found = bin_hit.step(sq_first(0, pass));
      if (found != 0xFFFFFFFFu) {
#pragma unroll
        for (uint32_t k = 0; k < kSqNpt; ++k) {
          if (k * 256 + tid != found) continue;  // (the owning lane's slot)
          left[k] -= 1;
#pragma unroll
          for (uint32_t r = 0; r < KSG_MAX_RES; ++r) fr[k][r] -= pod.req[r];
        }
        if (found == nodes) ++nodes;
        ++packed;
        bin = (int32_t)found;
      } else if (nodes < cap || fit_filter(SqLeft{e_fr, e_left}, &pod, (uint32_t)KSG_MAX_RES) != 0) {
        ++too_big;  // (nodes < cap: bin `nodes`, empty, was among the tested)
        bin = kScaleTooBig;
      } else {
        ++over_cap;
        bin = kScaleOverCap;
      }
    }
    if (bin < 0 && first_unpacked < 0) first_unpacked = (int32_t)i;
    if (PLAN && tid == 0) plan[i] = bin;
  }
  if (!PLAN && tid == 0) {
    ScaleUp s;
    s.nodes = (int32_t)nodes;
    s.packed = packed;
    s.closed = closed;
    s.too_big = too_big;
    s.over_cap = over_cap;
    s.first_unpacked = first_unpacked;
    s.base_pods = base_pods;
    s.reserved = 0;
    out[blockIdx.x] = s;
  }
}

namespace {
// The templates of `in` against the snapshot as the stream holds it: the launch
// inputs through the device buffer (behind them the open bytes), the structs (or
// the one template's bins) back through the pinned block, one synchronisation.
int scale_up_run(Engine& eng, const ScaleUpIn& in, ScaleUp* out, int32_t* plan, std::string& err) {
  Engine::Impl& I = *eng.impl();
  if (in.max_nodes < 1 || in.max_nodes > std::min(I.scale_max, kScaleMax)) {
    err = "scale_up: max_nodes outside [1, " + std::to_string(std::min(I.scale_max, kScaleMax)) + "]";
    return KSG_E_RANGE;
  }
  if (!in.n_templates) return KSG_OK;
  if (!out && !plan) return KSG_OK;  // (ksg_scale_up_plan of an empty list may come without a buffer: nothing to write)
  if (!sq_need_fit(I, "scale_up", err)) return KSG_E_INVALID;
  if (plan && in.n_templates != 1) {
    err = "scale_up: a plan is of one template";
    return KSG_E_RANGE;
  }
  for (uint32_t i = 0; i < in.n_templates; ++i)
    if (in.templates[i] >= I.N) {  // (host.cpp checked them against the local nodes)
      err = "scale_up: template outside the snapshot";
      return KSG_E_RANGE;
    }
  const uint32_t P = in.n_pods, T = in.n_templates;
  const size_t back_bytes = plan ? (size_t)P * sizeof(int32_t) : (size_t)T * sizeof(ScaleUp);
  if (!back_bytes) return KSG_OK;
  // the launch inputs: the base loads, the pod list, the templates; behind them the open bytes
  SqIn li;
  const size_t at_base = li.add<ScaleBase>(T), at_pods = li.add<uint32_t>(P), at_tmpl = li.add<uint32_t>(T);
  const size_t at_open = li.reserve((size_t)T * P);
  li.stage();
  if (P) std::memcpy(li.host<uint32_t>(at_pods), in.pods, (size_t)P * sizeof(uint32_t));
  std::memcpy(li.host<uint32_t>(at_tmpl), in.templates, (size_t)T * sizeof(uint32_t));
  for (uint32_t i = 0; i < T; ++i) {
    ScaleBase& b = li.host<ScaleBase>(at_base)[i];
    std::memcpy(b.req, in.base_req + (size_t)i * KSG_MAX_RES, sizeof(b.req));
    b.pods = in.base_pods[i];
    b.pad = 0;
  }
  uint32_t has_nodename = 0;
  for (int pos = 0; pos < I.F.n; ++pos) has_nodename |= I.F.plugins[pos] == KP_NODENAME;
  auto enqueue = [&](hipStream_t s) -> bool {
    const ScaleBase* d_base = li.dev<const ScaleBase>(at_base);
    const uint32_t* d_pods = li.dev<const uint32_t>(at_pods);
    const uint32_t* d_tmpl = li.dev<const uint32_t>(at_tmpl);
    uint8_t* d_open = li.dev<uint8_t>(at_open);
    for (uint32_t t0 = 0; P && t0 < T; t0 += 65535u)  // (grid.y <= 65535)
      hipLaunchKernelGGL(k_scale_open, dim3((P + 255) / 256, std::min(T - t0, 65535u)), dim3(256), 0, s, I.cluster(), I.F,
                         I.progs.p, I.prog_off_d.p, d_pods, P, d_tmpl + t0, has_nodename, d_open + (size_t)t0 * P);
    if (plan)
      hipLaunchKernelGGL(k_scale_pack<true>, dim3(1), dim3(256), 0, s, I.cluster(), I.progs.p, I.prog_off_d.p, d_pods, P,
                         d_tmpl, d_base, d_open, in.max_nodes, (ScaleUp*)nullptr, reinterpret_cast<int32_t*>(I.sq_out.p));
    else
      hipLaunchKernelGGL(k_scale_pack<false>, dim3(T), dim3(256), 0, s, I.cluster(), I.progs.p, I.prog_off_d.p, d_pods, P,
                         d_tmpl, d_base, d_open, in.max_nodes, reinterpret_cast<ScaleUp*>(I.sq_out.p), (int32_t*)nullptr);
    return true;
  };
  void* dst = plan ? (void*)plan : (void*)out;
  return sq_fetch(I, &li, back_bytes, 0, back_bytes, dst, enqueue, err) ? KSG_OK : KSG_E_DEVICE;
}
}  // namespace

}  // namespace ksg

extern "C" int ksg_scale_up(ksg_ctx* ctx, const uint32_t* pods, uint32_t n_pods, const uint32_t* templates,
                            uint32_t n_templates, uint32_t max_nodes, struct ksg_scale_up* out) {
  const bool args_ok = (pods || !n_pods) && (templates || !n_templates) && (out || !n_templates);
  return ksg::scale_up_call(ctx, pods, n_pods, templates, n_templates, max_nodes, args_ok, "scale_up", &ksg::scale_up_run,
                            out, nullptr);
}

extern "C" int ksg_scale_up_plan(ksg_ctx* ctx, const uint32_t* pods, uint32_t n_pods, uint32_t template_node,
                                 uint32_t max_nodes, int32_t* bin_out) {
  const bool args_ok = (pods || !n_pods) && (bin_out || !n_pods);
  return ksg::scale_up_call(ctx, pods, n_pods, &template_node, 1, max_nodes, args_ok, "scale_up_plan", &ksg::scale_up_run,
                            nullptr, bin_out);
}
