// tests/native/host_args_host.cpp -- csrc/host_args.h held to the one-sentence definition of each of its rules, over
// every small case: the header alone, no HIP, no GPU.  Built with AddressSanitizer and UBSan by tests/test_host_args.py.
//
//   spans_meet        "the byte sets intersect", over every pair of spans with start 0..6 and length 0..6, plus NULL
//   outputs_overlap   "one of the first nout spans meets any other span of the list", every list of up to four such
//                     spans, every nout
//   arrays_overlap    "any two spans of the list meet, except that with in_place the first and the last may start at
//                     one address", the same lists, both values of in_place
//   sorted neighbours csrc/solver.hip's form of "any two meet": after std::sort by operator<, two neighbours meet -- over
//                     every list of up to three non-empty spans (three is where a span between two others first exists)
//   outputs_alias     "a non-NULL output equals a non-NULL input or another output", every list of up to three outputs and
//                     up to three inputs drawn from {NULL, p, q, r}
//
// A byte set is a mask of the bytes of one buffer, so the brute-force side never compares addresses.  Exit status 0 and
// "every rule holds its definition", or the first case that differs and 1.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "host_args.h"

using namespace mms;

namespace {

constexpr int kStarts = 7, kLens = 7, kMaxList = 4;
char buffer[kStarts + kLens];

struct Case {
  const void* p;       // NULL, or buffer + start
  int start, len;      // start -1: NULL
  unsigned bytes;      // bit b: byte b of the buffer is in the array
  ByteSpan span;
};

std::vector<Case> all_cases() {
  std::vector<Case> v;
  for (int start = 0; start < kStarts; ++start)
    for (int len = 0; len < kLens; ++len)
      v.push_back({buffer + start, start, len, ((1u << len) - 1u) << start, byte_span(buffer + start, (size_t)len)});
  v.push_back({nullptr, -1, 3, 0u, byte_span(nullptr, 3)});      // a NULL array is none, whatever its extent
  return v;
}

[[noreturn]] void fail(const char* rule, const std::vector<const Case*>& list, int a, int b, bool want) {
  std::printf("%s differs: want %d, a = %d, b = %d, list", rule, (int)want, a, b);
  for (const Case* c : list) std::printf(" (start %d, len %d)", c->start, c->len);
  std::printf("\n");
  std::exit(1);
}

// ---- the definitions ------------------------------------------------------------------------------------------------
bool meet(const Case& a, const Case& b) { return (a.bytes & b.bytes) != 0; }

bool def_outputs_overlap(const std::vector<const Case*>& l, int nout) {
  for (int i = 0; i < nout; ++i)
    for (int j = 0; j < (int)l.size(); ++j)
      if (j != i && meet(*l[i], *l[j])) return true;
  return false;
}

bool def_arrays_overlap(const std::vector<const Case*>& l, bool in_place) {
  const int n = (int)l.size();
  for (int i = 0; i < n; ++i)
    for (int j = 0; j < n; ++j) {
      if (i == j || !meet(*l[i], *l[j])) continue;
      const bool first_and_last = (i == 0 && j == n - 1) || (j == 0 && i == n - 1);
      if (in_place && first_and_last && l[i]->p == l[j]->p) continue;
      return true;
    }
  return false;
}

bool def_outputs_alias(const std::vector<const void*>& outs, const std::vector<const void*>& ins) {
  for (size_t i = 0; i < outs.size(); ++i) {
    if (outs[i] == nullptr) continue;
    for (size_t j = 0; j < ins.size(); ++j)
      if (ins[j] != nullptr && ins[j] == outs[i]) return true;
    for (size_t j = 0; j < outs.size(); ++j)
      if (j != i && outs[j] == outs[i]) return true;
  }
  return false;
}

// ---- the sweeps -----------------------------------------------------------------------------------------------------
long long sweep_pairs(const std::vector<Case>& cases) {
  long long n = 0;
  for (const Case& a : cases)
    for (const Case& b : cases) {
      if (spans_meet(a.span, b.span) != meet(a, b)) fail("spans_meet", {&a, &b}, 0, 0, meet(a, b));
      ++n;
    }
  return n;
}

long long sweep_lists(const std::vector<Case>& cases) {
  const int C = (int)cases.size();
  long long lists = 0;
  std::vector<const Case*> l;
  ByteSpan spans[kMaxList];
  for (int n = 0; n <= kMaxList; ++n) {
    long long total = 1;
    for (int i = 0; i < n; ++i) total *= C;
    l.resize((size_t)n);
    for (long long code = 0; code < total; ++code) {
      long long c = code;
      for (int i = 0; i < n; ++i, c /= C) {
        l[(size_t)i] = &cases[(size_t)(c % C)];
        spans[i] = l[(size_t)i]->span;
      }
      for (int nout = 0; nout <= n; ++nout) {
        const bool want = def_outputs_overlap(l, nout);
        if (outputs_overlap(spans, n, nout) != want) fail("outputs_overlap", l, nout, 0, want);
      }
      for (int in_place = 0; in_place < 2; ++in_place) {
        const bool want = def_arrays_overlap(l, in_place != 0);
        if (arrays_overlap(spans, n, in_place != 0) != want) fail("arrays_overlap", l, in_place, 0, want);
      }
      ++lists;
    }
  }
  return lists;
}

long long sweep_sorted(const std::vector<Case>& cases) {
  std::vector<const Case*> full;
  for (const Case& c : cases)
    if (c.bytes) full.push_back(&c);
  const int C = (int)full.size();
  long long lists = 0;
  for (int n = 0; n <= 3; ++n) {
    long long total = 1;
    for (int i = 0; i < n; ++i) total *= C;
    std::vector<const Case*> l((size_t)n);
    for (long long code = 0; code < total; ++code) {
      long long c = code;
      ByteSpan spans[3];
      for (int i = 0; i < n; ++i, c /= C) {
        l[(size_t)i] = full[(size_t)(c % C)];
        spans[i] = l[(size_t)i]->span;
      }
      std::sort(spans, spans + n);
      bool got = false;
      for (int i = 1; i < n; ++i) got = got || spans_meet(spans[i - 1], spans[i]);
      const bool want = def_arrays_overlap(l, false);
      if (got != want) fail("sorted neighbours", l, 0, 0, want);
      ++lists;
    }
  }
  return lists;
}

long long sweep_alias() {
  static const char p = 0, q = 0, r = 0;
  const void* const values[4] = {nullptr, &p, &q, &r};
  long long n = 0;
  for (int no = 0; no <= 3; ++no)
    for (int ni = 0; ni <= 3; ++ni)
      for (int oc = 0; oc < (1 << (2 * no)); ++oc)
        for (int ic = 0; ic < (1 << (2 * ni)); ++ic) {
          std::vector<const void*> outs, ins;
          for (int i = 0; i < no; ++i) outs.push_back(values[(oc >> (2 * i)) & 3]);
          for (int i = 0; i < ni; ++i) ins.push_back(values[(ic >> (2 * i)) & 3]);
          const bool want = def_outputs_alias(outs, ins);
          bool got = outputs_alias(outs.data(), outs.size(), ins.data(), ins.size());
          if (no == 3 && ni == 3) {                     // the array form the sources call
            const void* const o[3] = {outs[0], outs[1], outs[2]};
            const void* const in[3] = {ins[0], ins[1], ins[2]};
            if (outputs_alias(o, in) != got) got = !want;
          }
          if (got != want) {
            std::printf("outputs_alias differs: want %d, outputs code %d of %d, inputs code %d of %d (two bits each: "
                        "0 NULL, 1 p, 2 q, 3 r)\n", (int)want, oc, no, ic, ni);
            std::exit(1);
          }
          ++n;
        }
  return n;
}

}  // namespace

int main() {
  const std::vector<Case> cases = all_cases();
  std::printf("spans %zu\n", cases.size());
  std::printf("pairs %lld\n", sweep_pairs(cases));
  std::printf("alias_lists %lld\n", sweep_alias());          // the short sweeps first: a changed rule is named at once
  std::printf("sorted_lists %lld\n", sweep_sorted(cases));
  std::printf("lists %lld\n", sweep_lists(cases));
  std::printf("every rule holds its definition\n");
  return 0;
}
