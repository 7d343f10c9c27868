// csrc/host_args.h -- what a host entry point judges about the ARRAYS of a call before it enqueues anything, once for
// every layer family: whether two of them share a byte (ByteSpan, spans_meet and the two list policies the families
// use) and whether an output IS another array of the call (outputs_alias: addresses alone, for the families whose
// extents the header does not promise).  The refusals include/*.h tabulates and tests/test_abi_*.py pin are these.
// Plain C++, no HIP: tests/native/host_args_host.cpp includes this file alone and holds every function to its
// one-sentence definition over every small case.
#ifndef MMS_HOST_ARGS_H_
#define MMS_HOST_ARGS_H_

#include <stddef.h>
#include <stdint.h>

namespace mms {

// [lo, hi) in bytes; lo == hi: no byte
struct ByteSpan {
  uintptr_t lo, hi;
};
// a NULL array is none: the empty span
inline ByteSpan byte_span(const void* p, size_t bytes) {
  const uintptr_t a = reinterpret_cast<uintptr_t>(p);
  const ByteSpan s = {a, p ? a + bytes : a};
  return s;
}
// the order csrc/solver.hip sorts by: an overlap among non-empty spans is then one between neighbours
inline bool operator<(const ByteSpan& a, const ByteSpan& b) { return a.lo != b.lo ? a.lo < b.lo : a.hi < b.hi; }

// whether a and b share a byte
inline bool spans_meet(const ByteSpan& a, const ByteSpan& b) {
  return a.lo != a.hi && b.lo != b.hi && a.lo < b.hi && b.lo < a.hi;
}

// whether one of the first `nout` spans of the list (the outputs) meets any other span of the list
inline bool outputs_overlap(const ByteSpan* s, int n, int nout) {
  for (int i = 0; i < nout; ++i)
    for (int j = i + 1; j < n; ++j)
      if (spans_meet(s[i], s[j])) return true;
  return false;
}

// whether any two spans of the list meet; with `in_place` the first and the last may start at one address
inline bool arrays_overlap(const ByteSpan* s, int n, bool in_place) {
  for (int i = 0; i < n; ++i)
    for (int j = i + 1; j < n; ++j) {
      if (in_place && i == 0 && j == n - 1 && s[i].lo == s[j].lo) continue;
      if (spans_meet(s[i], s[j])) return true;
    }
  return false;
}

// whether a non-NULL output is (the address of) a non-NULL input or another output
inline bool outputs_alias(const void* const* outputs, size_t nout, const void* const* inputs, size_t nin) {
  for (size_t i = 0; i < nout; ++i) {
    if (!outputs[i]) continue;
    for (size_t j = 0; j < nin; ++j)
      if (outputs[i] == inputs[j]) return true;
    for (size_t j = 0; j < i; ++j)
      if (outputs[i] == outputs[j]) return true;
  }
  return false;
}
template <size_t M, size_t K>
bool outputs_alias(const void* const (&outputs)[M], const void* const (&inputs)[K]) {
  return outputs_alias(outputs, M, inputs, K);
}

}  // namespace mms
#endif  // MMS_HOST_ARGS_H_
