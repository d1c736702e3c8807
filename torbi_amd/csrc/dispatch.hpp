// dispatch.hpp -- the one way from a runtime value (a state count, items per workgroup, a list length, a bool) to a template
// instance.  Every selector calls `f` with a std::integral_constant and returns what `f` returns; inside `f` the caller names
// its kernel instance ONCE (`auto *kernel = &ns::k<A, B>;`) and feeds the LDS grant, the occupancy query, the launch and the
// reported name from that one pointer and those constants.  Host only.
#pragma once

#include <type_traits>

// THE ladder from a state count to a backtrace instance: a lane of those kernels holds NQ float4 of a posterior row, which
// covers S <= 256 * NQ states.  Calls f(std::integral_constant<int, NQ>) for the first NQ of the list that covers S (the
// last one when none does: the callers have bounded S); without a list 2, 6, 8, 16 -- steps at 512, 1536 and 2048 states.
template <int NQ, int... MORE, class F>
inline auto by_state_count(int S, F &&f) {
    if constexpr (sizeof...(MORE) == 0) return f(std::integral_constant<int, NQ>());
    else if (S <= 256 * NQ) return f(std::integral_constant<int, NQ>());
    else return by_state_count<MORE...>(S, f);
}
// (overload resolution keeps the two apart: an int as first template argument does not fit `class F`, so a call with a list
// sees the form above alone, and a call without one cannot deduce NQ and sees the form below alone)
template <class F>
inline auto by_state_count(int S, F &&f) { return by_state_count<2, 6, 8, 16>(S, f); }

// f(std::integral_constant<int, V>) for the first V of the list that equals `v`, the last one when none does (the `default:`
// of a switch: every ladder keeps its fallback)
template <int V, int... MORE, class F>
inline auto by_value(int v, F &&f) {
    if constexpr (sizeof...(MORE) == 0) return f(std::integral_constant<int, V>());
    else if (v == V) return f(std::integral_constant<int, V>());
    else return by_value<MORE...>(v, f);
}

// f(std::true_type) or f(std::false_type)
template <class F>
inline auto by_flag(bool b, F &&f) { return b ? f(std::true_type()) : f(std::false_type()); }

// THE tile rule: items per workgroup of a kernel whose workgroup shares one pass over a matrix among G items -- from `max_g`,
// halved while fits(G) (the LDS rows of G items) does not hold, then while the B items give fewer than `wanted` workgroups
// (`per_item_workgroups`: workgroups of one group of items)
template <class Fits>
inline int items_per_workgroup(int max_g, int B, int per_item_workgroups, int wanted, Fits &&fits) {
    int G = max_g;
    while (G > 1 && !fits(G)) G >>= 1;
    while (G > 1 && (long long)((B + G - 1) / G) * per_item_workgroups < wanted) G >>= 1;
    return G;
}
