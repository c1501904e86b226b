// How the launchers of dg_api.h become Python functions: shared by the bindings file of every
// HIP module (bindings.cpp for `_dghip`, <name>_bindings.cpp for the small `_dg<name>`).
//
// Tensors cross the boundary as raw device addresses (tensor.data_ptr()), tables of host
// integers as the address of the host array, and the HIP stream as its handle
// (torch.cuda.current_stream().cuda_stream): the Python layer (deep_go_amd/ops) owns allocation,
// shape checks and stream choice, and every launcher validates the shape invariants it relies
// on before touching the GPU.  A launcher's error becomes
// RuntimeError("<name>: <hipGetErrorString>").
//
// A binding that forwards all its arguments is derived from the declaration by Bind<&fn>; one
// that pins some arguments (the nullptr of a _bf16 twin, say) is an explicit lambda over P, S
// and check.
#pragma once
#include <pybind11/pybind11.h>

#include <stdexcept>
#include <string>
#include <type_traits>

#include "dg_api.h"

namespace py = pybind11;

namespace {

template <typename T>
T* P(uintptr_t v) {
  return reinterpret_cast<T*>(v);
}
[[maybe_unused]] hipStream_t S(uintptr_t v) { return reinterpret_cast<hipStream_t>(v); }

[[maybe_unused]] void check(hipError_t e, const char* what) {
  if (e != hipSuccess)
    throw std::runtime_error(std::string(what) + ": " + hipGetErrorString(e));
}

// How one C parameter crosses the boundary: pointers (hipStream_t is one) as integers,
// everything else as itself.
template <typename T>
struct Arg {
  using py = T;
  static T to(T v) { return v; }
};
template <typename T>
struct Arg<T*> {
  using py = uintptr_t;
  static T* to(uintptr_t v) { return reinterpret_cast<T*>(v); }
};

// Bind<&dg_f>::def(m, "f"): the Python function f with dg_f's parameter list; a hipError_t
// result is checked (RuntimeError "f: <hipGetErrorString>"), any other is returned.
template <auto Fn>
struct Bind;
template <typename R, typename... A, R (*Fn)(A...)>
struct Bind<Fn> {
  static void def(py::module_& m, const char* name, const char* doc = "") {
    m.def(name, [name](typename Arg<A>::py... a) {
      if constexpr (std::is_same_v<R, hipError_t>)
        check(Fn(Arg<A>::to(a)...), name);
      else
        return Fn(Arg<A>::to(a)...);
    }, doc);
  }
};

}  // namespace
