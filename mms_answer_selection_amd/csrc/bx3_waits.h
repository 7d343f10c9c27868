// csrc/bx3_waits.h -- what a loader wave of bx3_kernel (bx3_gemm.h) may leave in flight at each of its counted
// s_waitcnt vmcnt(N): the one definition.  Plain constexpr C++ (no HIP header, no intrinsic): the kernel takes its
// immediates from these functions, and tests/native/bx3_waits_host.cpp replays a loader wave's instruction stream on
// the host with the same functions and proves the invariants below for every PER, ksteps and side count.
//
// A loader wave's vector-memory stream (PER operand LDS-DMAs per k-step; NS = 6 ring slots):
//   issue(0) .. issue(NS - 2);
//   for j = 0 .. ksteps:   wait(j); barrier j; side(j) = [store(j - 3)] [request(j)];  issue(j + NS - 1)
//   finish:                vmcnt(0); the stores the loop did not reach; then request, vmcnt(0), store one index at a time
// (every part only where it exists: step < ksteps, index < cnt).  A side request is 2 LDS-DMAs into slot (index % 4)
// of the side ring, a side store reads that slot back and is 1 global store.
//
// The hardware assumption under every count (panel_gemm.h rests on the same): as far as vmcnt is concerned a wave's
// vector-memory operations, stores included, retire in the order they were issued -- vmcnt(N) returns when all but the
// youngest N have.  The side ring's slice a wave reads is the slice its own DMAs wrote, so the wave's own wait orders it.
//
// Invariants (the host program asserts them at every point of every run):
//   A  operands:   at barrier j every DMA of operand steps j and j + 1 has retired;
//   B  side ring:  store(i) reads its slot only after both DMAs of request(i) have retired, in the loop and in finish;
//                  request(i) is issued only after store(i - 4), the slot's previous reader; every index is requested
//                  and stored exactly once;
//   C  no over-wait: while the schedule leaves three operand steps in flight (out == 3) a wait forces nothing to retire
//                  that is younger than both what A and B need and the first DMA of the oldest of those three steps,
//                  except for the bucket's rounding (< kBx3WaitBucket operations), and nothing at all when the side
//                  count is a multiple of the bucket -- as in steady state, where three whole steps stay in flight;
//   D  range:      every immediate fits vmcnt's six bits.
// The tails (out < 3: the last NS - 1 barriers of a workgroup, or all of them when ksteps < NS - 1) and finish do not
// count side operations at all: out * PER, then 0.  That waits for more than A and B need -- sound, and left so: C
// bounds the tail's length instead of its waits.
#ifndef MMS_BX3_WAITS_H_
#define MMS_BX3_WAITS_H_

namespace mms {

constexpr int kBx3NS = 6;             // the ring depth these counts are derived for (Bx3Geom::NS)
constexpr int kBx3InFlight = 3;       // operand steps left in flight across a barrier in steady state (NS - 3)
constexpr int kBx3SideLag = 3;        // side step j stores the index side step j - 3 requested
constexpr int kBx3SideRing = 4;       // slots of the side ring
constexpr int kBx3SideStoreOps = 1, kBx3SideRequestOps = 2;
constexpr int kBx3WaitBucket = 3;     // a wait's immediate is a compile-time operand: side counts come in steps of 3
constexpr int kBx3WaitBuckets = 6;    // 0, PER, 2 PER, 3 PER, 3 PER + 3, 3 PER + 6
constexpr int kBx3VmcntMax = 63;

// ---- the operand schedule -------------------------------------------------------------------------------------------
constexpr int bx3_prologue_steps(int ksteps) { return ksteps < kBx3NS - 1 ? ksteps : kBx3NS - 1; }
// the step issued behind barrier j (into the slot of step j - 1, which that barrier released), or -1
constexpr int bx3_issue_behind_barrier(int j, int ksteps) { return j + kBx3NS - 1 < ksteps ? j + kBx3NS - 1 : -1; }
struct Bx3Sched { int hi, need, out; };   // at barrier j: youngest step issued, step that must have landed, hi - need
constexpr Bx3Sched bx3_sched(int j, int ksteps) {
  const int last = ksteps - 1;
  const int hi = j + kBx3NS - 2 < last ? j + kBx3NS - 2 : last, need = j + 1 < last ? j + 1 : last;
  return {hi, need, hi - need};
}

// ---- the side ledger: what side step j of a wave with cnt indices issues ----------------------------------------------
constexpr bool bx3_side_stores(int j, int cnt) { return j >= kBx3SideLag && j - kBx3SideLag < cnt; }   // store(j - 3)
constexpr bool bx3_side_requests(int j, int cnt) { return j >= 0 && j < cnt; }                         // request(j)
constexpr int bx3_side_step_ops(int j, int cnt) {
  return (bx3_side_stores(j, cnt) ? kBx3SideStoreOps : 0) + (bx3_side_requests(j, cnt) ? kBx3SideRequestOps : 0);
}
// Side operations YOUNGER than the oldest operand step barrier j leaves in flight (step j + 2, issued behind side(j - 3)):
// those of side steps j - 2 and j - 1.  Side step j - 3 is older than that step; it holds request(j - 3), which
// store(j - 3) is about to read, so it must not be counted (B) -- and waiting for it reaches into no operand DMA (C).
constexpr int bx3_side_ops_younger_than_in_flight(int j, int cnt) {
  return bx3_side_step_ops(j - 2, cnt) + bx3_side_step_ops(j - 1, cnt);
}

// ---- the wait at barrier j: bucket (which bx3_wait_vm<N> instantiation) and immediate ----------------------------------
// A bucket only rounds the side count DOWN: the wait covers more, never less.
constexpr int bx3_wait_bucket(int out, int side_younger) {
  if (out < kBx3InFlight) return out;                                    // tails: side operations not counted
  const int b = kBx3InFlight + side_younger / kBx3WaitBucket;
  return b < kBx3WaitBuckets ? b : kBx3WaitBuckets - 1;
}
constexpr int bx3_wait_imm(int PER, int bucket) {
  return bucket <= kBx3InFlight ? bucket * PER : kBx3InFlight * PER + (bucket - kBx3InFlight) * kBx3WaitBucket;
}

// ---- finish(steps_done): the loop ran side steps 0 .. steps_done - 1 --------------------------------------------------
// After its vmcnt(0): indices [first, requested) were requested by the loop and not stored by it -- stored at once;
// indices [requested, cnt) are requested, waited for (vmcnt(0)) and stored one at a time.
constexpr int bx3_finish_first(int steps_done) { return steps_done > kBx3SideLag ? steps_done - kBx3SideLag : 0; }
constexpr int bx3_finish_requested(int steps_done, int cnt) { return steps_done < cnt ? steps_done : cnt; }

static_assert(kBx3InFlight == kBx3NS - 3 && kBx3SideLag <= kBx3InFlight && kBx3SideRing > kBx3SideLag,
              "request(j - 3) is older than step j + 2 = j + NS - 4, and its slot is not requested again before store(j - 3)");
static_assert(2 * (kBx3SideStoreOps + kBx3SideRequestOps) == (kBx3WaitBuckets - 1 - kBx3InFlight) * kBx3WaitBucket,
              "the top bucket holds two whole side steps: steady state is exact");

}  // namespace mms

#endif  // MMS_BX3_WAITS_H_
