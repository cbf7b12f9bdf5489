// Set drain (ksg_drain_sets / ksg_drain_prefixes / ksg_drain_set_plan,
// include/ksg.h): can several nodes be removed together -- the subjects of all
// of them re-placed one after another outside the set, each counted on its
// destination before the next is judged, from whichever member it came.  Part of
// the engine's translation unit (engine.hip includes it after drain.hip).
//
//   k_drain_set<false>  one block of 256 threads per set, every set of a call in
//                 one launch.  k_drain's chain (drain.hip: the subject loop, the
//                 tile walk that ends at the first tile with a hit, the rows
//                 reloaded when the walk enters another tile, the first-hit step
//                 written out as there) with two changes, below: who is excluded
//                 as a destination, and how the overlay is searched.  Thread 0
//                 also keeps the list position of the first node with an unplaced
//                 subject; with the skipped subjects' it gives first_blocked.
//   k_drain_set<true>   the same body for one set with a store of {bound, dest}
//                 per subject (ksg_drain_set_plan); subjects beyond the cap get -2.
//
// Membership.  The host hands over the set's members sorted by node, each with
// its position in the caller's list, and a position limit: a node is in the set
// when it is found and its position is below the limit (the set size; k + 1 for
// prefix k, whose sets all read the one sorted list of the whole call).  The
// block copies them into LDS once, padded to KSG_DRAIN_SET_NODES with a node no
// snapshot holds.  Only a node that passes the whole walk is looked up: a node
// outside [lowest member, highest member] is none, the others take a binary
// search of 7 halvings over the 128 entries.
//
// Overlay.  As drain.hip's it is the simulation's own placements, private to the
// block and in LDS for the reason given there (a block's vector stores are not
// coherent with its reads through the scalar cache).  A set's subjects come from
// up to 128 nodes and spread further than one node's, so the distinct
// destinations are found through an open-addressed hash table instead of a
// linear search: 2 x cap slots (cap: the effective KSG_DRAIN_MAX, a power of
// two), home slot = local node index & (2 x cap - 1), linear probing with
// wrap-around, 0xFFFFFFFF empty.  A slot holds the node and the index of its
// entry; the entries -- pod count and KSG_MAX_RES int64 requests, as in drain.hip
// -- are dense, one per distinct destination, so the table doubles the keys
// only and the whole stays one static allocation under 64 KB.  At most cap
// subjects are placed, so the table is never more than half full: a probe meets
// an empty slot within 2 x cap steps, and the loop is bounded by the table size
// besides.  Thread 0 alone inserts, between the two barriers that frame the
// overlay update; a lookup runs only for a node that passes against its rows
// alone, and the overlay only lowers what is left.
//
// Forward progress: drain.hip's argument.  The only waits are block barriers;
// the subject loop's bound, the tile loop's bound and the found-break are
// block-uniform (the set's descriptor and the tile's hit are read from LDS after
// a barrier, cap and the tile count are kernel arguments); the probe and the
// search hold no barrier.  Subjects <= cap, tiles <= ceil(N / kSqTile), a probe
// <= 2 x cap slots, the search 7 steps.  No block reads what another block
// wrote; nothing is launched persistently.
#include "../../include/ksg.h"

namespace ksg {

using DrainSet = struct ::ksg_drain_set;
static_assert(sizeof(DrainSet) == 32 && offsetof(DrainSet, placed) == 8 && offsetof(DrainSet, first_unplaced) == 20 &&
                  offsetof(DrainSet, first_blocked) == 24 && offsetof(DrainSet, dest_nodes) == 28,
              "the kernel stores the struct's own layout");
static_assert(sizeof(DrainSetDesc) == 32 && sizeof(DrainSetMember) == 8, "the kernel reads the host's structs");
constexpr uint32_t kDrainSetNodes = KSG_DRAIN_SET_NODES;
static_assert(kDrainSetNodes == 128, "the member search is 7 halvings");
constexpr uint32_t kDrainSetSlots = 2 * kDrainMax;
static_assert(kDrainMax <= 0x8000 && (kDrainMax & (kDrainMax - 1)) == 0, "a slot's entry index is 16 bits");
constexpr size_t kDrainSetLds = kDrainSetSlots * (sizeof(uint32_t) + sizeof(uint16_t)) +
                                kDrainMax * (sizeof(int32_t) + KSG_MAX_RES * sizeof(int64_t)) +
                                kDrainSetNodes * sizeof(DrainSetMember) + 16 * sizeof(uint32_t);
static_assert(kDrainSetLds < 64 * 1024, "the overlay and the members are one static LDS allocation under 64 KB");

// sets: entry blockIdx.x is the block's; members / off / bidx / spos: the lists its ranges index (off: the
// subjects' offsets into the store); cap: a power of two <= kDrainMax
template <bool PLAN>
__global__ __launch_bounds__(256) void k_drain_set(DevCluster C, DevProfile F, const uint8_t* __restrict__ store,
                                                   const DrainSetDesc* __restrict__ sets,
                                                   const DrainSetMember* __restrict__ members,
                                                   const uint64_t* __restrict__ off, const int32_t* __restrict__ bidx,
                                                   const uint32_t* __restrict__ spos, uint32_t cap, uint32_t tiles,
                                                   DrainSet* out, DrainMove* plan) {
  __shared__ int64_t ov_req[kDrainMax][KSG_MAX_RES];  // per distinct destination: requests added
  __shared__ int32_t ov_cnt[kDrainMax];               // pods added
  __shared__ uint32_t ov_key[kDrainSetSlots];         // the table: local node index, 0xFFFFFFFF empty
  __shared__ uint16_t ov_ent[kDrainSetSlots];         // its entry
  __shared__ uint32_t mem_node[kDrainSetNodes];       // the members, ascending, padded with 0xFFFFFFFF
  __shared__ uint32_t mem_pos[kDrainSetNodes];
  __shared__ uint32_t hit[3];
  __shared__ DrainSetDesc s_set;
  const uint32_t tid = threadIdx.x;
  const uint32_t mask = 2 * cap - 1;
  if (tid == 0) {
    s_set = sets[blockIdx.x];
    hit[0] = hit[1] = hit[2] = 0xFFFFFFFFu;
  }
  for (uint32_t i = tid; i <= mask; i += 256) ov_key[i] = 0xFFFFFFFFu;
  __syncthreads();
  const uint32_t start = s_set.s_start, subjects = s_set.s_count, limit = s_set.limit;
  const uint32_t n_mem = s_set.m_count < kDrainSetNodes ? s_set.m_count : kDrainSetNodes;
  if (tid < kDrainSetNodes) {
    const bool have = tid < n_mem;
    const DrainSetMember m = have ? members[s_set.m_start + tid] : DrainSetMember{0xFFFFFFFFu, 0xFFFFFFFFu};
    mem_node[tid] = m.node;
    mem_pos[tid] = m.pos;
  }
  __syncthreads();
  // (no member: an empty range, lo > hi)
  const uint32_t mem_lo = n_mem ? mem_node[0] : 1u, mem_hi = n_mem ? mem_node[n_mem - 1] : 0u;
  const uint32_t n_sim = subjects < cap ? subjects : cap;
  int64_t fr[kSqNpt][KSG_MAX_RES];
  int32_t left[kSqNpt];
  uint32_t loaded = 0xFFFFFFFFu, it = 0;
  int32_t placed = 0, unplaced = 0, first_unplaced = -1, first_blocked = -1, n_ent = 0;  // (thread 0's)
#pragma unroll 1
  for (uint32_t s = 0; s < n_sim; ++s) {
    const ProgView V = view(store + off[start + s]);
    const ksg_prog* h = V.h;
    SqPod pod;
    pod.flags = h->flags;
#pragma unroll
    for (uint32_t r = 0; r < KSG_MAX_RES; ++r) pod.req[r] = r < C.R ? h->req[r] : 0;
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
        if (sq_live(C, V, n)) {
          const uint32_t code = sq_walk<kPmPlaced>(C, F, V, n, [&]() -> uint32_t {
            const uint32_t alone = fit_filter(SqLeft{fr[k], left[k]}, &pod, (uint32_t)KSG_MAX_RES);
            if (alone) return alone;
            for (uint32_t i = 0; i <= mask; ++i) {  // (ends at an empty slot: the table is at most half full)
              const uint32_t slot = (n + i) & mask;
              const uint32_t key = ov_key[slot];
              if (key == 0xFFFFFFFFu) break;
              if (key != n) continue;
              const uint32_t j = ov_ent[slot];
              int64_t f[KSG_MAX_RES];
#pragma unroll
              for (uint32_t r = 0; r < KSG_MAX_RES; ++r) f[r] = fr[k][r] - ov_req[j][r];
              return fit_filter(SqLeft{f, left[k] - ov_cnt[j]}, &pod, (uint32_t)KSG_MAX_RES);
            }
            return 0;
          });
          pass = code == KSG_FILTER_PASS;
          if (pass && n >= mem_lo && n <= mem_hi) {  // a member is no destination
            uint32_t lo = 0;
#pragma unroll
            for (uint32_t half = kDrainSetNodes / 2; half; half >>= 1)
              if (mem_node[lo + half] <= n) lo += half;
            pass = !(mem_node[lo] == n && mem_pos[lo] < limit);
          }
        }
        const unsigned long long b = __ballot(pass);
        if (b && first == 0xFFFFFFFFu)  // (wave-uniform; a lane's nodes ascend with k)
          first = t * kSqTile + k * 256 + (tid & ~63u) + (uint32_t)__ffsll((long long)b) - 1;
      }
      // (keep in step with SqFirstHit::step, snapshot_query.hip, which carries the argument; k_drain)
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
        if (!unplaced++) {
          first_unplaced = b;
          first_blocked = (int32_t)spos[start + s];
        }
      } else {
        ++placed;
        uint32_t slot = found & mask;
        while (ov_key[slot] != found && ov_key[slot] != 0xFFFFFFFFu) slot = (slot + 1) & mask;  // (half full at most)
        if (ov_key[slot] == 0xFFFFFFFFu) {  // (n_ent <= s < cap)
          ov_key[slot] = found;
          ov_ent[slot] = (uint16_t)n_ent;
          ov_cnt[n_ent] = 0;
#pragma unroll
          for (uint32_t r = 0; r < KSG_MAX_RES; ++r) ov_req[n_ent][r] = 0;
          ++n_ent;
        }
        const uint32_t j = ov_ent[slot];
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
    if (first_blocked < 0 && n_sim < subjects) first_blocked = (int32_t)spos[start + n_sim];
    DrainSet d;
    d.pods = s_set.pods;
    d.daemon = s_set.daemon;
    d.placed = placed;
    d.unplaced = unplaced;
    d.skipped = (int32_t)(subjects - n_sim);
    d.first_unplaced = first_unplaced;
    d.first_blocked = first_blocked;
    d.dest_nodes = n_ent;
    out[blockIdx.x] = d;
  }
}

namespace {
// The sets of `in` against the snapshot as the stream holds it: the launch inputs
// through the device buffer, the structs (or the one set's moves) back through
// the pinned block, one synchronisation.  The ranges are checked here once more:
// the kernel indexes the lists with them.
int drain_set_run(Engine& eng, const DrainSetIn& in, DrainSet* out, DrainMove* plan, std::string& err) {
  Engine::Impl& I = *eng.impl();
  const uint32_t N = I.N;
  if (!sq_need_fit(I, "drain_sets", err)) return KSG_E_INVALID;
  if (!in.n_sets || (plan && in.n_sets != 1)) {
    err = "drain_sets: sets";
    return KSG_E_RANGE;
  }
  for (uint32_t i = 0; i < in.n_sets; ++i) {
    const DrainSetDesc& d = in.sets[i];
    if (d.m_count > kDrainSetNodes || (size_t)d.m_start + d.m_count > in.n_members ||
        (size_t)d.s_start + d.s_count > in.n_subjects) {
      err = "drain_sets: a set outside its lists";
      return KSG_E_RANGE;
    }
  }
  for (uint32_t i = 0; i < in.n_members; ++i)
    if (in.members[i].node >= N) {
      err = "drain_sets: nodes outside the snapshot";
      return KSG_E_RANGE;
    }
  const uint32_t total = in.n_subjects;
  const size_t back_bytes = plan ? (size_t)in.sets[0].s_count * sizeof(DrainMove) : (size_t)in.n_sets * sizeof(DrainSet);
  if (!back_bytes) return KSG_OK;
  // the launch inputs: the sets, the members and the subjects' positions, then the subjects (drain.hip)
  SqIn li;
  size_t at_sets = li.add<DrainSetDesc>(in.n_sets), at_mem = li.add<DrainSetMember>(in.n_members),
         at_pos = li.add<uint32_t>(total), at_off, at_bidx;
  if (!drain_subjects(I, li, in.subj, total, "drain_sets", at_off, at_bidx, err)) return KSG_E_STATE;
  std::memcpy(li.host<DrainSetDesc>(at_sets), in.sets, (size_t)in.n_sets * sizeof(DrainSetDesc));
  if (in.n_members) std::memcpy(li.host<DrainSetMember>(at_mem), in.members, (size_t)in.n_members * sizeof(DrainSetMember));
  if (total) std::memcpy(li.host<uint32_t>(at_pos), in.subj_pos, (size_t)total * sizeof(uint32_t));
  const uint32_t cap = std::min(I.drain_max, kDrainMax), tiles = (N + kSqTile - 1) / kSqTile;
  return drain_fetch(I, li, back_bytes, in.n_sets, out, plan, err, [&](auto is_plan, dim3 grid, hipStream_t s) {
    hipLaunchKernelGGL(k_drain_set<decltype(is_plan)::value>, grid, dim3(256), 0, s, I.cluster(), I.F, I.vstore.p,
                       li.dev<const DrainSetDesc>(at_sets), li.dev<const DrainSetMember>(at_mem),
                       li.dev<const uint64_t>(at_off), li.dev<const int32_t>(at_bidx), li.dev<const uint32_t>(at_pos), cap,
                       tiles, drain_out<DrainSet>(I, !is_plan), drain_out<DrainMove>(I, is_plan));
  });
}
}  // namespace

}  // namespace ksg

extern "C" int ksg_drain_sets(ksg_ctx* ctx, const uint32_t* nodes, const uint32_t* set_start, uint32_t n_sets,
                              struct ksg_drain_set* out) {
  return ksg::drain_set_call(ctx, nodes, set_start, n_sets, !n_sets || (set_start && out), "drain_sets",
                             &ksg::drain_set_run, out, nullptr, 0, nullptr);
}

extern "C" int ksg_drain_prefixes(ksg_ctx* ctx, const uint32_t* nodes, uint32_t n, struct ksg_drain_set* out) {
  return ksg::drain_set_call(ctx, nodes, nullptr, n, !n || (nodes && out), "drain_prefixes", &ksg::drain_set_run, out,
                             nullptr, 0, nullptr);
}

extern "C" int ksg_drain_set_plan(ksg_ctx* ctx, const uint32_t* nodes, uint32_t n, struct ksg_drain_move* out,
                                  uint32_t cap, uint32_t* n_out) {
  if (n_out) *n_out = 0;
  return ksg::drain_set_call(ctx, nodes, nullptr, n, !n || (nodes && out && n_out), "drain_set_plan", &ksg::drain_set_run,
                             nullptr, out, cap, n_out);
}
