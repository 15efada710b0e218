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

// Runtime split-K count -> a consumer kernel's SP (partials.h): sp_dispatch<1, 2, 4, 8>(S, f)
// calls f(Int<S>{}) when S is one of the listed counts, else f(Int<0>{}), the runtime loop.
// sp_dispatch_exact has no fallback: it returns false (f not called) for an unlisted S.
template <int... SP, class F>
bool sp_dispatch_exact(int S, F&& f) {
  return ((S == SP && (f(Int<SP>{}), true)) || ...);
}
template <int... SP, class F>
void sp_dispatch(int S, F&& f) {
  if (!sp_dispatch_exact<SP...>(S, f)) f(Int<0>{});
}

template <class T, int N>
constexpr int table_size(const T (&)[N]) { return N; }

}  // namespace xgk
