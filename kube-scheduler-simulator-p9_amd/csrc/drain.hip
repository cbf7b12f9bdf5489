// Drain simulation (ksg_drain / ksg_drain_plan, include/ksg.h): can a node be
// emptied -- its bound pods re-placed one after another, each on the lowest node
// that admits it and counted there before the next is judged.  Part of the
// engine's translation unit (engine.hip includes it after bound_fit.hip).
//
//   k_drain<false>  one block of 256 threads per candidate node x.  The subjects
//                 (the launch inputs: per candidate a range of a list of bound
//                 indices and victim-store offsets, ascending bound index) are
//                 taken in order.  For a subject the block walks the nodes in
//                 ascending tiles of kSqTile: a lane computes the codes of its
//                 kSqNpt nodes as k_bound_fit does, the source lowered by the
//                 overlay's entry for the node if it has one; x itself is no
//                 destination.  The tile's lowest passing node comes off the
//                 ballots and through the three rotating LDS words as sq_first
//                 and SqFirstHit::step (snapshot_query.hip) do it, one barrier
//                 per tile step, written out here: called from this kernel they
//                 give the same answers, but the listing moves throughout and
//                 ksg_drain measured 2.5 to 6 % slower on loose clusters.  The
//                 walk ends at the first tile with a hit: first fit costs a loose
//                 cluster one tile per subject, not N nodes.  The rows are loaded
//                 when the walk enters another tile than the one the registers
//                 hold.  Thread 0 then counts the subject on its destination in
//                 the overlay, and the block barriers.  At the end thread 0
//                 stores the 32-byte struct: nothing is accumulated across blocks.
//   k_drain<true>   the same body for one candidate with a store of {bound, dest}
//                 per subject (ksg_drain_plan); subjects beyond the cap get -2.
//
// The overlay is the drain's own placements, private to the block, in LDS (not
// in global memory: a block's vector stores are not coherent with its reads
// through the scalar cache): the distinct destinations, and per destination the
// pods and the requests of the R columns added so far.  A node that passes
// against its rows alone looks its entry up by a linear search over the distinct
// destinations (broadcast LDS reads; first fit keeps them few) and runs
// fit_filter once more against the lowered rows.  The overlay only lowers what
// is left, so a node that fails without it fails with it.  Not tuned: see
// DESIGN.md "Drain simulation".
//
// Forward progress: snapshot_query.hip's argument.  The subject loop's bound, the
// tile loop's bound and the found-break are block-uniform: the subject count and
// the tile's hit are read from LDS after a barrier, the tile count is a kernel
// argument.  Subjects <= KSG_DRAIN_MAX, tiles <= ceil(N / kSqTile), the overlay
// search <= the subjects so far.
#include "../../include/ksg.h"

namespace ksg {

using Drain = struct ::ksg_drain;  // (the function of the same name hides the struct's)
using DrainMove = struct ::ksg_drain_move;
static_assert(KSG_DRAIN_MAX == kDrainMax, "the header's cap is the overlay's size");
static_assert(sizeof(Drain) == 32 && offsetof(Drain, placed) == 8 && offsetof(Drain, first_unplaced) == 20 &&
                  offsetof(Drain, reserved) == 28,
              "the kernel stores the struct's own layout");
static_assert(sizeof(DrainMove) == 8 && offsetof(DrainMove, dest) == 4, "");
// one candidate's launch input: its subjects are entries [start, start + subjects) of the lists
struct DrainCand {
  uint32_t start, subjects;
  int32_t pods, daemon;
};
constexpr size_t kDrainLds =
    kDrainMax * (sizeof(uint32_t) + sizeof(int32_t) + KSG_MAX_RES * sizeof(int64_t)) + 8 * sizeof(uint32_t);
static_assert(kDrainLds < 64 * 1024, "the overlay is one static LDS allocation under 64 KB");

// cand: entry 0 is the launch's first candidate, local node first_node; off / bidx: the subjects' offsets
// into the store and bound indices; cap <= kDrainMax
template <bool PLAN>
__global__ __launch_bounds__(256) void k_drain(DevCluster C, DevProfile F, const uint8_t* __restrict__ store,
                                               const DrainCand* __restrict__ cand, const uint64_t* __restrict__ off,
                                               const int32_t* __restrict__ bidx, uint32_t first_node, uint32_t cap,
                                               uint32_t tiles, Drain* out, DrainMove* plan) {
  __shared__ int64_t ov_req[kDrainMax][KSG_MAX_RES];  // per distinct destination: requests added
  __shared__ uint32_t ov_dest[kDrainMax];             // the distinct destinations (local node index)
  __shared__ int32_t ov_cnt[kDrainMax];               // pods added
  __shared__ uint32_t ov_n;
  __shared__ uint32_t hit[3];
  __shared__ uint32_t s_start, s_subjects;
  const uint32_t tid = threadIdx.x;
  const uint32_t x = first_node + blockIdx.x;
  if (tid == 0) {
    const DrainCand c = cand[blockIdx.x];
    s_start = c.start;
    s_subjects = c.subjects;
    ov_n = 0;
    hit[0] = hit[1] = hit[2] = 0xFFFFFFFFu;
  }
  __syncthreads();
  const uint32_t start = s_start, subjects = s_subjects;
  const uint32_t n_sim = subjects < cap ? subjects : cap;
  int64_t fr[kSqNpt][KSG_MAX_RES];
  int32_t left[kSqNpt];
  uint32_t loaded = 0xFFFFFFFFu, it = 0;
  int32_t placed = 0, unplaced = 0, first_unplaced = -1;  // (thread 0's)
#pragma unroll 1
  for (uint32_t s = 0; s < n_sim; ++s) {
    const ProgView V = view(store + off[start + s]);
    const ksg_prog* h = V.h;
    SqPod pod;
    pod.flags = h->flags;
#pragma unroll
    for (uint32_t r = 0; r < KSG_MAX_RES; ++r) pod.req[r] = r < C.R ? h->req[r] : 0;
    const uint32_t nd = ov_n;  // (after the barrier that followed its last update)
    uint32_t found = 0xFFFFFFFFu;
#pragma unroll 1
    for (uint32_t t = 0; t < tiles; ++t) {
      const uint32_t base = t * kSqTile + tid;
      if (t != loaded) {  // (block-uniform)
        sq_rows(C, base, fr, left);
        loaded = t;
      }
      uint32_t first = 0xFFFFFFFFu;
#pragma unroll
      for (uint32_t k = 0; k < kSqNpt; ++k) {
        const uint32_t n = base + k * 256;
        bool pass = false;
        if (n != x && sq_live(C, V, n)) {
          const uint32_t code = sq_walk<kPmPlaced>(C, F, V, n, [&]() -> uint32_t {
            const uint32_t alone = fit_filter(SqLeft{fr[k], left[k]}, &pod, (uint32_t)KSG_MAX_RES);
            if (alone) return alone;
            for (uint32_t j = 0; j < nd; ++j) {
              if (ov_dest[j] != n) continue;
              int64_t f[KSG_MAX_RES];
#pragma unroll
              for (uint32_t r = 0; r < KSG_MAX_RES; ++r) f[r] = fr[k][r] - ov_req[j][r];
              return fit_filter(SqLeft{f, left[k] - ov_cnt[j]}, &pod, (uint32_t)KSG_MAX_RES);
            }
            return 0;
          });
          pass = code == KSG_FILTER_PASS;
        }
        const unsigned long long b = __ballot(pass);
        if (b && first == 0xFFFFFFFFu)  // (wave-uniform; a lane's nodes ascend with k)
          first = t * kSqTile + k * 256 + (tid & ~63u) + (uint32_t)__ffsll((long long)b) - 1;
      }
      // (keep in step with SqFirstHit::step, snapshot_query.hip, which carries the argument; sq_first above)
      if (first != 0xFFFFFFFFu && lane0()) atomicMin(&hit[it % 3], first);
      __syncthreads();
      found = hit[it % 3];
      if (tid == 0) hit[(it + 2) % 3] = 0xFFFFFFFFu;
      ++it;
      if (found != 0xFFFFFFFFu) break;  // (block-uniform)
    }
    if (tid == 0) {
      const int32_t b = bidx[start + s];
      if (found == 0xFFFFFFFFu) {
        if (!unplaced++) first_unplaced = b;
      } else {
        ++placed;
        uint32_t j = 0;
        while (j < nd && ov_dest[j] != found) ++j;
        if (j == nd) {  // (nd <= s < kDrainMax)
          ov_dest[j] = found;
          ov_cnt[j] = 0;
#pragma unroll
          for (uint32_t r = 0; r < KSG_MAX_RES; ++r) ov_req[j][r] = 0;
          ov_n = nd + 1;
        }
        ov_cnt[j] += 1;
#pragma unroll
        for (uint32_t r = 0; r < KSG_MAX_RES; ++r) ov_req[j][r] += pod.req[r];
      }
      if (PLAN) plan[s] = DrainMove{b, found == 0xFFFFFFFFu ? -1 : (int32_t)(C.goff + found)};
    }
    __syncthreads();
  }
  if (PLAN) {
    for (uint32_t s = n_sim + tid; s < subjects; s += 256) plan[s] = DrainMove{bidx[start + s], -2};
  } else if (tid == 0) {
    const DrainCand c = cand[blockIdx.x];
    Drain d;
    d.pods = c.pods;
    d.daemon = c.daemon;
    d.placed = placed;
    d.unplaced = unplaced;
    d.skipped = (int32_t)(subjects - n_sim);
    d.first_unplaced = first_unplaced;
    d.dest_nodes = (int32_t)ov_n;
    d.reserved = 0;
    out[blockIdx.x] = d;
  }
}

namespace {
// A drain call's subjects as launch inputs (drain_run, and drain_set_run in drain_set.hip), behind the
// arrays the caller has laid out in `li`: their victim-store offsets (at_off) and bound indices (at_bidx)
// are laid out, `li` is staged and both are filled.  false: err is set (KSG_E_STATE).
bool drain_subjects(const Engine::Impl& I, SqIn& li, const int32_t* subj, uint32_t total, const char* what,
                    size_t& at_off, size_t& at_bidx, std::string& err) {
  at_off = li.add<uint64_t>(total);
  at_bidx = li.add<int32_t>(total);
  li.stage();
  uint64_t* h_off = li.host<uint64_t>(at_off);
  if (total) std::memcpy(li.host<int32_t>(at_bidx), subj, (size_t)total * sizeof(int32_t));
  for (uint32_t i = 0; i < total; ++i) {
    const int32_t b = subj[i];
    if (b < 0 || (size_t)b >= I.vstore_off.size()) {  // (host.cpp ensured the store for this very bound list)
      err = std::string(what) + ": bound pod outside the victim store";
      return false;
    }
    h_off[i] = I.vstore_off[(size_t)b];
  }
  return true;
}

// A drain call's launch and round trip.  launch(is_plan, grid, stream) enqueues the kernel's <true>
// instantiation on one block for a plan (is_plan: std::true_type), its <false> instantiation on `blocks`
// otherwise; either writes I.sq_out, and back_bytes of it come back through the pinned block into plan
// or out, one synchronisation.
template <class T>
T* drain_out(Engine::Impl& I, bool used) {  // (null for the pointer an instantiation does not touch)
  return used ? reinterpret_cast<T*>(I.sq_out.p) : nullptr;
}
template <class Launch>
int drain_fetch(Engine::Impl& I, SqIn& li, size_t back_bytes, uint32_t blocks, void* out, DrainMove* plan,
                std::string& err, Launch launch) {
  auto enqueue = [&](hipStream_t s) -> bool {
    if (plan) launch(std::true_type{}, dim3(1), s);
    else launch(std::false_type{}, dim3(blocks), s);
    return true;
  };
  return sq_fetch(I, &li, back_bytes, 0, back_bytes, plan ? (void*)plan : out, enqueue, err) ? KSG_OK : KSG_E_DEVICE;
}

// The candidates of `in` against the snapshot as the stream holds it: the launch
// inputs through the device buffer, the structs (or the one candidate's moves)
// back through the pinned block, one synchronisation.
int drain_run(Engine& eng, const DrainIn& in, Drain* out, DrainMove* plan, std::string& err) {
  Engine::Impl& I = *eng.impl();
  if (!sq_need_fit(I, "drain", err)) return KSG_E_INVALID;
  const uint32_t total = in.start[in.count];
  if ((size_t)in.first_node + in.count > I.N || (plan && in.count != 1)) {
    err = "drain: candidates outside the snapshot";
    return KSG_E_RANGE;
  }
  const size_t back_bytes = plan ? (size_t)total * sizeof(DrainMove) : (size_t)in.count * sizeof(Drain);
  if (!back_bytes) return KSG_OK;
  // the launch inputs: the candidates, then the subjects
  SqIn li;
  size_t at_cand = li.add<DrainCand>(in.count), at_off, at_bidx;
  if (!drain_subjects(I, li, in.subj, total, "drain", at_off, at_bidx, err)) return KSG_E_STATE;
  DrainCand* h_cand = li.host<DrainCand>(at_cand);
  for (uint32_t c = 0; c < in.count; ++c)
    h_cand[c] = DrainCand{in.start[c], in.start[c + 1] - in.start[c], in.pods[c], in.daemon[c]};
  const uint32_t cap = std::min(I.drain_max, kDrainMax), tiles = (I.N + kSqTile - 1) / kSqTile;
  return drain_fetch(I, li, back_bytes, in.count, out, plan, err, [&](auto is_plan, dim3 grid, hipStream_t s) {
    hipLaunchKernelGGL(k_drain<decltype(is_plan)::value>, grid, dim3(256), 0, s, I.cluster(), I.F, I.vstore.p,
                       li.dev<const DrainCand>(at_cand), li.dev<const uint64_t>(at_off), li.dev<const int32_t>(at_bidx),
                       in.first_node, cap, tiles, drain_out<Drain>(I, !is_plan), drain_out<DrainMove>(I, is_plan));
  });
}
}  // namespace

}  // namespace ksg

extern "C" int ksg_drain(ksg_ctx* ctx, uint32_t first_node, uint32_t count, struct ksg_drain* out) {
  return ksg::drain_call(ctx, first_node, count, out != nullptr, "drain", &ksg::drain_run, out, nullptr, 0, nullptr);
}

extern "C" int ksg_drain_plan(ksg_ctx* ctx, uint32_t node, struct ksg_drain_move* out, uint32_t cap, uint32_t* n_out) {
  if (n_out) *n_out = 0;
  return ksg::drain_call(ctx, node, 1, out != nullptr && n_out != nullptr, "drain_plan", &ksg::drain_run, nullptr, out, cap,
                         n_out);
}
