// Runtime cfg -> compile-time table row: cfg_dispatch<N>(cfg, f) calls
// f(std::integral_constant<int, C>{}) for the C in 0 .. N - 1 equal to cfg, so a launcher
// reads its template arguments from a constexpr table row `TABLE[decltype(c)::value]`.
// Returns false (f not called) when cfg is outside the table.
#pragma once

#include <type_traits>
#include <utility>

namespace xgk {

template <int V>
using Int = std::integral_constant<int, V>;

template <class F, int... C>
bool cfg_dispatch_seq(int cfg, F&& f, std::integer_sequence<int, C...>) {
  return ((cfg == C && (f(std::integral_constant<int, C>{}), true)) || ...);
}
template <int N, class F>
bool cfg_dispatch(int cfg, F&& f) {
  return cfg_dispatch_seq(cfg, f, std::make_integer_sequence<int, N>{});
}

template <class T, int N>
constexpr int table_size(const T (&)[N]) { return N; }

}  // namespace xgk
