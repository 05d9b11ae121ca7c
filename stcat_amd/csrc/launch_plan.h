// Launch plans: the launch sequence of a composite node of the hot path (backbone forward / backward, the
// spatial-temporal encoder, the two decoders, the heads — models/pipeline.py:52-121 in the reference's call order)
// recorded ONCE per input shape as a flat list of C-ABI calls and replayed by stcat_plan_run() in one host call.
// Round 2 issued every one of the ~1700 launches of a step as its own Python -> ctypes call (host floor 29 ms per
// step); a replay costs one hipLaunchKernel per op.
//
// A recorded call is (entry point, argument words).  Every argument of the launch entry points is a device pointer,
// an int / long, a float or the stream, so one 64-bit word per argument holds it and a thunk generated from the entry
// point's own C type unpacks the words again (no libffi, no per-function code).  Pointers into tensors the caller
// passes in per step ("externals": the node's inputs, parameters, upstream gradients) are patched through a
// relocation list (word, external index, byte offset) at the top of every replay; every other pointer was allocated
// from the plan's private memory pool during recording and stays valid for the life of the plan.  Streams are slots
// (0 = the caller's current stream, 1.. = the side streams of the recording); WAIT ops carry the event that orders
// one slot behind another (the weight-gradient stream of the backbone's backward).  YIELD ops hand control back to the
// host in the middle of a replay (the data-parallel reducer's early bucket delivery, stcat_amd/dist.py).
#pragma once

#include <cstdint>
#include <cstring>
#include <type_traits>
#include <utility>
#include <vector>

namespace stcat_plan {

typedef int (*ThunkFn)(const uint64_t*);

struct FnEntry {
  const char* name;
  const char* kinds;  // one letter per argument (entry_points.h)
  ThunkFn call;       // nullptr: not recordable
  int nargs;
};

template <class T>
inline T arg_of(uint64_t w) {
  if constexpr (std::is_pointer<T>::value) {
    return reinterpret_cast<T>(static_cast<uintptr_t>(w));
  } else if constexpr (std::is_floating_point<T>::value) {
    float f;
    const uint32_t u = (uint32_t)w;
    memcpy(&f, &u, 4);
    return (T)f;
  } else {
    return (T)(int64_t)w;
  }
}

template <class F, F f>
struct Thunk;
template <class... A, int (*f)(A...)>
struct Thunk<int (*)(A...), f> {
  template <size_t... I>
  static int go(const uint64_t* w, std::index_sequence<I...>) {
    return f(arg_of<A>(w[I])...);
  }
  static int call(const uint64_t* w) { return go(w, std::index_sequence_for<A...>{}); }
  static constexpr int nargs = (int)sizeof...(A);
};

// The kind letters of entry_points.h against an entry point's own C type: kinds_match<decltype(&fn)>(kinds).  The
// letters are what the hosts build their argument types from and what a recorder packs the argument words by, so a
// letter that disagrees with the prototype must not compile.
constexpr int kinds_len(const char* k) { return *k ? 1 + kinds_len(k + 1) : 0; }
constexpr bool same_str(const char* a, const char* b) { return *a == *b && (!*a || same_str(a + 1, b + 1)); }

template <class T>
constexpr bool kind_is(char k, bool last) {
  switch (k) {
    case 'i': return std::is_same<T, int>::value;
    case 'l': return std::is_same<T, long>::value;
    case 'f': return std::is_same<T, float>::value;
    case 'u': return std::is_same<T, unsigned long long>::value;
    case 'S': return std::is_same<T, const char*>::value;
    case 's': return std::is_same<T, void*>::value && last;
    case 'p':
    case 'P': return std::is_pointer<T>::value && !std::is_same<T, const char*>::value;
    default: return false;
  }
}

template <class F>
struct KindsOf;
template <class R, class... A>
struct KindsOf<R (*)(A...)> {
  template <size_t... I>
  static constexpr bool args(const char* k, std::index_sequence<I...>) {
    return (kind_is<A>(k[I], I + 1 == sizeof...(A)) && ...);
  }
  // every entry point returns int; `returns_handle` marks the one that returns a void* (stcat_plan_create)
  static constexpr bool match(const char* k, bool returns_handle) {
    return (returns_handle ? std::is_same<R, void*>::value : std::is_same<R, int>::value) &&
           kinds_len(k) == (int)sizeof...(A) && args(k, std::index_sequence_for<A...>{});
  }
};
template <class F>
constexpr bool kinds_match(const char* kinds, bool returns_handle = false) {
  return KindsOf<F>::match(kinds, returns_handle);
}

// recordable: a stream-ordered launch (the stream comes last) that takes no host pointer
constexpr bool recordable(const char* k) {
  bool host = false;
  char last = 0;
  for (; *k; ++k) { host = host || *k == 'P'; last = *k; }
  return last == 's' && !host;
}
template <bool rec, class F, F f>
constexpr ThunkFn thunk_if() {
  if constexpr (rec) return &Thunk<F, f>::call;
  else return nullptr;
}
enum OpKind : uint8_t { OP_CALL = 0, OP_WAIT = 1, OP_MEMSET = 2, OP_YIELD = 3 };

struct Op {
  uint8_t kind;
  uint8_t slot;    // CALL / MEMSET: stream slot the op is issued on; WAIT: the slot that waits
  uint8_t slot2;   // WAIT: the slot whose queued work is waited for
  uint8_t pad;
  int32_t fn;      // CALL: index into the entry-point table; YIELD: tag handed back to the host
  uint32_t arg0;   // CALL: first argument word; MEMSET: word of the pointer (bytes in the next word); WAIT: event index
  int32_t nargs;
  int32_t stream_arg;  // CALL: argument position that receives the slot's stream (-1: none)
};

struct Reloc {
  uint32_t word;
  uint32_t ext;
  uint64_t off;
};

struct Plan {
  std::vector<Op> ops;
  std::vector<uint64_t> words;
  std::vector<Reloc> relocs;
  std::vector<void*> events;  // hipEvent_t, created on first replay
  int n_ext = 0;
  int n_slots = 1;
  long replays = 0;
};

}  // namespace stcat_plan
