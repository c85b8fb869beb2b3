// Run-time values -> template arguments, the one idiom every launcher uses (plain C++17, no HIP).
//
//   pick(miss, f, axis...)            f(c1, c2, ...) with one constant per axis, in the order given;
//                                     an axis is Of<list>{v} (v not listed: pick returns miss), or
//                                     Or<fallback, list>{v} (v not listed: the fallback), or Flag{b}
//   pick_tuple(Table<Tup<..>,..>{}, miss, f, v...)
//                                     f(c1, c2, ...) for the listed tuple equal to (v...), else miss
//
// A constant is a std::integral_constant: a callable `[&](auto g, auto nt) { return launch<g, nt>(..); }`
// uses it as a template argument. A launcher and its occupancy query hand their callables to the
// same pick over the same lists, so they cannot name different instantiations.
#pragma once

#include <type_traits>

namespace netcsum {
namespace dsp {

template <auto V>
using Const = std::integral_constant<decltype(V), V>;

template <auto... Vs>
struct Of {                                    // one of Vs, else no match
    long long v;
    template <typename R, typename G>
    R visit(R miss, G&& g) const {
        R r = miss;
        (void)((v == (long long)Vs && ((r = g(Const<Vs>{})), true)) || ...);
        return r;
    }
};

template <auto FB, auto... Vs>
struct Or {                                    // one of Vs, else FB
    long long v;
    template <typename R, typename G>
    R visit(R miss, G&& g) const {
        R r = miss;
        const bool hit = ((v == (long long)Vs && ((r = g(Const<Vs>{})), true)) || ...);
        return hit ? r : g(Const<FB>{});
    }
};

using Flag = Of<false, true>;

template <typename R, typename F>
R pick(R, F&& f) {
    return f();
}

template <typename R, typename F, typename A, typename... Rest>
R pick(R miss, F&& f, A axis, Rest... rest) {
    return axis.visit(miss, [&](auto c) { return pick(miss, [&](auto... cs) { return f(c, cs...); }, rest...); });
}

template <auto... Vs>
struct Tup {};

template <typename... Ts>
struct Table {};

template <auto... Vs, typename... V>
bool tup_is(Tup<Vs...>, V... v) {
    return ((v == (V)Vs) && ...);
}

template <auto... Vs, typename F>
auto tup_call(Tup<Vs...>, F&& f) {
    return f(Const<Vs>{}...);
}

template <typename... Ts, typename R, typename F, typename... V>
R pick_tuple(Table<Ts...>, R miss, F&& f, V... v) {
    R r = miss;
    (void)((tup_is(Ts{}, v...) && ((r = tup_call(Ts{}, f)), true)) || ...);
    return r;
}

}  // namespace dsp
}  // namespace netcsum
