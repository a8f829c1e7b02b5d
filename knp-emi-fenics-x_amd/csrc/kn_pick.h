// From a run-time integer to a template argument: the one dispatcher of the assembly launchers.  Host only,
// no HIP: plain C++17, as with_model in ode_host.h is for the membrane models.
//
// Which instantiations of a kernel exist is said by a constexpr predicate next to the kernel (knp_rows_built, ...); a
// launcher nests one kn_pick per template axis and guards the innermost body with `if constexpr (..._built(...))`, so a
// combination outside the predicate is neither compiled nor reachable, and the launcher reports it instead of running
// some default.  Everything resolves at compile time: a pick is a chain of integer compares, as the switch it replaces.
// (g++ 11 fails on `decltype(l)::value` of an ENCLOSING generic lambda's parameter inside a nested one; code it has to
// compile names the constant at its own level -- `constexpr int L = decltype(l)::value;` -- as tests/native/kn_pick_check.cpp does.)
#pragma once

#include <type_traits>

// calls f(std::integral_constant<int, V>{}) for the first V of Vs equal to v: true; no such V: false, f is not called
template <int... Vs, class F>
bool kn_pick(int v, F&& f) {
  return ((v == Vs ? (f(std::integral_constant<int, Vs>{}), true) : false) || ...);
}
