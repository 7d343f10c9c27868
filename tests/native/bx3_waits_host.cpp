// tests/native/bx3_waits_host.cpp -- the counted waits of bx3_kernel's loader waves (csrc/bx3_waits.h), proved on the
// host.  A loader wave's vector-memory instruction stream is replayed as an in-order queue of outstanding operations
// (operand DMA of step s, side request i, side store i); a wait vmcnt(N) retires the oldest until at most N remain,
// and nothing retires otherwise -- the latest completion the hardware allows.  Invariants A-D of the header are
// asserted at every point of every run, for every PER the kernels pass, ksteps 1 .. 48 and side counts 0 .. ksteps + 8.
// One line per violated invariant, exit status 1.
//
//   bx3_waits_host                  the header's rule
//   bx3_waits_host --rule parent    the rule the kernel had before the header (side steps j - 3 .. j - 1 all counted as
//                                   "may stay in flight", buckets of 9 / 6 / 0): reports B and nothing else -- the check
//                                   that this model sees a store reading a slot whose request is still outstanding
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "bx3_waits.h"

using namespace mms;

namespace {

// A rule: the immediate at barrier j, and (where out == 3) how many of the side operations it counts its bucket rounded away
struct Wait { int imm, rounded; };
Wait ledger_wait(int PER, int j, int ksteps, int cnt) {
  const int out = bx3_sched(j, ksteps).out, so = bx3_side_ops_younger_than_in_flight(j, cnt);
  const int imm = bx3_wait_imm(PER, bx3_wait_bucket(out, so));
  return {imm, out >= kBx3InFlight ? kBx3InFlight * PER + so - imm : 0};
}
Wait parent_wait(int PER, int j, int ksteps, int cnt) {
  const int out = bx3_sched(j, ksteps).out;
  if (out < 3) return {out * PER, 0};
  const int so = bx3_side_step_ops(j - 3, cnt) + bx3_side_step_ops(j - 2, cnt) + bx3_side_step_ops(j - 1, cnt);
  const int b = so >= 9 ? 9 : so >= 6 ? 6 : 0;
  return {3 * PER + b, so - b};
}
struct Rule { const char* name; Wait (*wait)(int, int, int, int); int bucket; };
const Rule kRules[] = {{"ledger", ledger_wait, kBx3WaitBucket}, {"parent", parent_wait, 6}};

struct Report {
  long count[4] = {0, 0, 0, 0};
  std::string first[4];
  void fail(char inv, const char* fmt, ...) {
    const int k = inv - 'A';
    if (count[k]++) return;
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    first[k] = buf;
  }
};

enum Kind { OPERAND, REQUEST, STORE };

struct Wave {
  const int PER, ksteps, cnt;
  Report& rep;
  std::vector<Kind> q;                 // every operation issued so far, oldest first; q[0 .. retired) have retired
  size_t retired = 0;
  std::vector<size_t> op_end, req_end; // queue length behind the last DMA of operand step s / of request i (0: not issued)
  std::vector<int> nreq, nstore;
  size_t b_need = 0;                   // queue position the last store needed retired

  Wave(int PER_, int ksteps_, int cnt_, Report& r)
      : PER(PER_), ksteps(ksteps_), cnt(cnt_), rep(r), op_end(ksteps_, 0), req_end(cnt_, 0), nreq(cnt_, 0), nstore(cnt_, 0) {}

  void fail(char inv, int j, const std::string& what) {
    rep.fail(inv, "PER=%d ksteps=%d cnt=%d %s: %s", PER, ksteps, cnt, j >= 0 ? ("barrier " + std::to_string(j)).c_str() : "finish",
             what.c_str());
  }
  void wait(int n) {
    if (q.size() - retired > (size_t)n) retired = q.size() - (size_t)n;
  }
  void issue(int s) {
    q.insert(q.end(), (size_t)PER, OPERAND);
    op_end[s] = q.size();
  }
  void request(int i, int j) {
    if (i < 0 || i >= cnt) return fail('B', j, "request(" + std::to_string(i) + ") is no index of this wave");
    if (i >= kBx3SideRing && !nstore[i - kBx3SideRing])
      fail('B', j, "request(" + std::to_string(i) + ") overwrites the slot store(" + std::to_string(i - kBx3SideRing) + ") has not read");
    q.insert(q.end(), (size_t)kBx3SideRequestOps, REQUEST);
    req_end[i] = q.size();
    ++nreq[i];
  }
  void store(int i, int j) {
    if (i < 0 || i >= cnt) return fail('B', j, "store(" + std::to_string(i) + ") is no index of this wave");
    if (!nreq[i]) fail('B', j, "store(" + std::to_string(i) + ") without a request");
    else if (req_end[i] > retired)
      fail('B', j, "store(" + std::to_string(i) + ") reads its slot with " + std::to_string(req_end[i] - retired) +
                       " operation(s) up to request(" + std::to_string(i) + ")'s DMAs still outstanding");
    b_need = req_end[i];
    q.insert(q.end(), (size_t)kBx3SideStoreOps, STORE);
    ++nstore[i];
  }

  void run(const Rule& rule) {
    for (int s = 0; s < bx3_prologue_steps(ksteps); ++s) issue(s);
    int tails = 0, side_steps = 0, prev_rounded = 0;
    for (int j = 0; j <= ksteps; ++j) {
      const Bx3Sched sc = bx3_sched(j, ksteps);
      const Wait w = rule.wait(PER, j, ksteps, cnt);
      const int imm = w.imm;
      if (imm < 0 || imm > kBx3VmcntMax) fail('D', j, "vmcnt(" + std::to_string(imm) + ")");
      const size_t before = retired;
      wait(imm);
      const size_t after = retired;
      size_t operands_left = 0;
      for (size_t k = after; k < q.size(); ++k) operands_left += q[k] == OPERAND;
      // A: the barrier
      for (int s = j; s <= j + 1 && s < ksteps; ++s)
        if (!op_end[s] || op_end[s] > after)
          fail('A', j, "operand step " + std::to_string(s) + " has not landed behind vmcnt(" + std::to_string(imm) + ")");
      // the side step (B is asserted inside)
      b_need = 0;
      if (bx3_side_stores(j, cnt)) store(j - kBx3SideLag, j);
      if (bx3_side_requests(j, cnt)) request(j, j);
      ++side_steps;
      // C: what the wait forced beyond A's and B's needs
      if (sc.out >= kBx3InFlight) {
        size_t floor_ = op_end[sc.need] > b_need ? op_end[sc.need] : b_need;
        const size_t oldest_in_flight = op_end[sc.need + 1] - (size_t)PER;    // operations older than step need + 1's first DMA
        if (oldest_in_flight > floor_) floor_ = oldest_in_flight;
        if (before > floor_) floor_ = before;
        const size_t excess = after > floor_ ? after - floor_ : 0;
        if (w.rounded < 0 || w.rounded >= rule.bucket)
          fail('C', j, "vmcnt(" + std::to_string(imm) + ") is not its side count rounded down within a bucket");
        else if (excess > (size_t)w.rounded)
          fail('C', j, "vmcnt(" + std::to_string(imm) + ") forces " + std::to_string(excess) + " operation(s) of the steps left in flight, " +
                           std::to_string(w.rounded) + " of them the bucket's rounding");
        else if (!w.rounded && !prev_rounded && operands_left != (size_t)(kBx3InFlight * PER))   // two exact waits in a row
          fail('C', j, std::to_string(operands_left) + " operand DMAs left in flight, not three whole steps");
        prev_rounded = w.rounded;
      } else {
        ++tails;
      }
      const int s = bx3_issue_behind_barrier(j, ksteps);
      if (s >= 0) issue(s);
    }
    if (tails > kBx3NS - 1) fail('C', ksteps, std::to_string(tails) + " barriers whose wait does not count side operations");
    // finish
    if (cnt) {
      wait(0);
      const int requested = bx3_finish_requested(side_steps, cnt);
      for (int i = bx3_finish_first(side_steps); i < requested; ++i) store(i, -1);
      for (int i = requested; i < cnt; ++i) {
        request(i, -1);
        wait(0);
        store(i, -1);
      }
    }
    for (int s = 0; s < ksteps; ++s)
      if (!op_end[s]) fail('A', -1, "operand step " + std::to_string(s) + " never issued");
    for (int i = 0; i < cnt; ++i)
      if (nreq[i] != 1 || nstore[i] != 1)
        fail('B', -1, "index " + std::to_string(i) + " requested " + std::to_string(nreq[i]) + " and stored " + std::to_string(nstore[i]) + " time(s)");
    if (!cnt && q.size() != (size_t)ksteps * (size_t)PER) fail('B', -1, "side operations without a side job");
  }
};

}  // namespace

int main(int argc, char** argv) {
  const Rule* rule = &kRules[0];
  for (int i = 1; i < argc; ++i) {
    if (!strcmp(argv[i], "--rule") && i + 1 < argc && (!strcmp(argv[i + 1], "ledger") || !strcmp(argv[i + 1], "parent"))) {
      rule = &kRules[!strcmp(argv[++i], "parent")];
    } else {
      fprintf(stderr, "usage: %s [--rule ledger|parent]\n", argv[0]);
      return 2;
    }
  }
  // PER: NTW 1 .. 5 image blocks of a plane; 4 half A blocks + 1 Y prefetch; 8 fp32 A blocks + 1 Y prefetch
  static const int kPer[] = {1, 2, 3, 4, 5, 9};
  Report rep;
  long runs = 0;
  for (int PER : kPer)
    for (int ksteps = 1; ksteps <= 48; ++ksteps)
      for (int cnt = 0; cnt <= ksteps + 8; ++cnt, ++runs) Wave(PER, ksteps, cnt, rep).run(*rule);
  static const char* const kName[4] = {"A (operands landed at the barrier)", "B (side ring)", "C (no over-wait)", "D (immediate <= 63)"};
  bool bad = false;
  for (int k = 0; k < 4; ++k)
    if (rep.count[k]) {
      bad = true;
      printf("%c violated, %ld time(s): %s; first: %s\n", 'A' + k, rep.count[k], kName[k], rep.first[k].c_str());
    }
  if (!bad) printf("bx3_waits_host ok: rule %s, %ld runs, invariants A-D hold\n", rule->name, runs);
  return bad ? 1 : 0;
}
