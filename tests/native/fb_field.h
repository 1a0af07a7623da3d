// Fb<P>: the signed-limb field Fs<P> of fields.cuh with its preconditions checked at every call.
//
// fields.cuh states in prose what each operator wants of its operands (limb range, |value| in multiples of p) and what it returns.
// The group law (ecu.cuh, ecq.cuh) is correct only if every call site honours that, and no input can steer the intermediates of an
// addition to the worst limb pattern all at once, so no test on values can see a call site that does not.  Fb carries, next to the
// real Fs value it computes with, an ENVELOPE that depends on the history of operations alone and not on the values:
//   lo, hi : every limb below the top one is in [lo, hi]   (the L of the prose is max(-lo, hi));
//   V      : |value| < V * p, in units of 2^-16 p and rounded up; V = 0 says the value is 0.
// Every operation first checks its precondition on the operand envelopes, then computes with Fs, then gives the result the envelope
// the rule of fields.cuh states -- so a law instantiated over Fb and run once per branch, with the input envelopes widened to the
// class invariant, proves by induction that no chain of its operations ever leaves the contract, for every input.
// A violated precondition is recorded (operation, operand, envelopes, the caller's site tag, the quad role), never aborted on.
// The rules live in fb::rule() below and nowhere else; fb_rule() of fu_check.cpp exports them to tests/test_fieldu.py, which checks
// each of them against big-integer arithmetic at the extreme of its precondition.
#pragma once
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <mutex>
#include <string>
#include <vector>
#include "../../ark_plonk_amd/csrc/fields.cuh"

namespace fb {

// ---- the constants of the rules, each with the place that states it
constexpr int64_t VU = 1 << 16;                               // one p, in the units V is held in
constexpr int64_t STRICT_LO = -(1ll << 29);                   // fields.cuh "strict": v[i] in [-2^29, 2^29)
constexpr int64_t STRICT_HI = (1ll << 29) - 1;
constexpr int64_t ALMOST = (1ll << 29) + 2;                   // fields.cuh "almost": |v[i]| <= 2^29 + 2 -- what the sums return, what the products take
constexpr int64_t SUM2_LIMIT = (1ll << 31) - (1ll << 29);     // fields.cuh normalize(): |in| < 2^31 - 2^29 for add / sub / dbl
constexpr int64_t I32_MIN = -(1ll << 31), I32_MAX = (1ll << 31) - 1;   // fields.cuh normalize_wide(): "limbs anywhere in int32" for add3 / sub_sum3
constexpr int64_t MUL_V = 12 * VU;                            // fields.cuh: inputs of mul / sqr / dot2 have |value| < 12p
constexpr int64_t DOT2_VV = 288 * VU * VU;                    // fields.cuh dot2: |a||b| + |c||d| < 288 p^2
constexpr int64_t RP_OVER_P = 512;                            // tools/gen_constants.py signed_struct(): asserts R' // p >= 512 for every modulus
constexpr int64_t REDUCED_V = 2 * VU;                         // fields.cuh is_zero_mod_reduced / canon_floor: value in (-2p, 2p)

struct Env {
    int64_t lo, hi, V;
};
inline bool inside(const Env& e, const Env& of) { return e.lo >= of.lo && e.hi <= of.hi && e.V <= of.V; }
inline Env join(const Env& a, const Env& b) { return Env{a.lo < b.lo ? a.lo : b.lo, a.hi > b.hi ? a.hi : b.hi, a.V > b.V ? a.V : b.V}; }

enum Op : int {
    OP_ZERO = 0, OP_ONE, OP_ADD, OP_DBL, OP_ADD3, OP_SUB, OP_SUB_SUM3, OP_NEG, OP_MUL, OP_SQR, OP_DOT2,
    OP_IS_ZERO_MOD_REDUCED, OP_LIMB0_OF_ZERO_MOD, OP_CANONICAL_LT2P, OP_LIMBS_ZERO, OP_WORDS, OP_COUNT
};
inline const char* op_name(int op) {
    static const char* n[OP_COUNT] = {"zero", "one", "add", "dbl", "add3", "sub", "sub_sum3", "neg", "mul", "sqr", "dot2",
                                      "is_zero_mod_reduced", "limb0_of_zero_mod", "canonical_lt2p", "limbs_zero", "split_words"};
    return op >= 0 && op < OP_COUNT ? n[op] : "?";
}
inline int op_arity(int op) {
    static const int n[OP_COUNT] = {0, 0, 2, 1, 3, 2, 4, 1, 2, 1, 4, 1, 1, 1, 1, 0};
    return op >= 0 && op < OP_COUNT ? n[op] : -1;
}

struct RuleOut {
    bool ok;
    int operand;          // the operand that misses the precondition; -1: the raw limb sum of all of them
    const char* why;
    Env res;
};

// THE rule table.  e: the operand envelopes; tp: an upper bound of p / 2^(30 (NL - 1)) + 1/2 (the top digit of p, plus one).
// The top limb of a value with |value| < V p and lower limbs below 2^30 - 1 in magnitude is at most ceil(V tp) in magnitude: the sums
// check it like any other limb.  The products need no check of their own for it: V <= 12 puts it below (12p >> 30 (NL - 1)) + 2, which
// is what the column bound of gen_constants.py is proved for.
inline RuleOut rule(int op, const Env* e, int64_t tp, int64_t words_v = 0) {
    RuleOut r{true, -1, "", Env{0, 0, 0}};
    auto top = [&](int64_t V) { return (V * tp + VU - 1) / VU + 1; };
    auto fail = [&](int operand, const char* why) {
        if (r.ok) {
            r.ok = false;
            r.operand = operand;
            r.why = why;
        }
    };
    auto product_operand = [&](int i) {                     // fields.cuh: "almost-balanced limbs, |value| < 12p"
        if (e[i].lo < -ALMOST || e[i].hi > ALMOST) fail(i, "limbs beyond 2^29 + 2");
        if (e[i].V > MUL_V) fail(i, "|value| not below 12p");
    };
    auto product_v = [&](int64_t vv) {                      // |a||b| / R' + |m| p / R' with the balanced quotient |m| <= R'/2 (1 + 2^-30): one unit on top of 1/2
        return (vv + RP_OVER_P * VU - 1) / (RP_OVER_P * VU) + VU / 2 + 1;
    };
    auto sum2 = [&](int64_t lo, int64_t hi, int64_t t, int64_t V) {
        if (hi >= SUM2_LIMIT || lo <= -SUM2_LIMIT || t >= SUM2_LIMIT) fail(-1, "raw limb sum not below 2^31 - 2^29");
        r.res = Env{-ALMOST, ALMOST, V};
    };
    auto sum_wide = [&](int64_t lo, int64_t hi, int64_t t, int64_t V) {
        if (hi > I32_MAX || lo < I32_MIN || t + 2 > I32_MAX) fail(-1, "raw limb sum outside int32");
        r.res = Env{-ALMOST, ALMOST, V};
    };
    switch (op) {
    case OP_ZERO: r.res = Env{0, 0, 0}; break;
    case OP_ONE: r.res = Env{STRICT_LO, STRICT_HI, VU}; break;                  // R' mod p in balanced digits
    case OP_WORDS: r.res = Env{STRICT_LO, STRICT_HI, words_v}; break;            // a non-negative integer below 2^(32 SAT)
    case OP_ADD: sum2(e[0].lo + e[1].lo, e[0].hi + e[1].hi, top(e[0].V) + top(e[1].V), e[0].V + e[1].V); break;
    case OP_SUB: sum2(e[0].lo - e[1].hi, e[0].hi - e[1].lo, top(e[0].V) + top(e[1].V), e[0].V + e[1].V); break;
    case OP_DBL: sum2(2 * e[0].lo, 2 * e[0].hi, 2 * top(e[0].V), 2 * e[0].V); break;
    case OP_ADD3:
        sum_wide(e[0].lo + e[1].lo + e[2].lo, e[0].hi + e[1].hi + e[2].hi, top(e[0].V) + top(e[1].V) + top(e[2].V), e[0].V + e[1].V + e[2].V);
        break;
    case OP_SUB_SUM3:
        sum_wide(e[0].lo - e[1].hi - e[2].hi - e[3].hi, e[0].hi - e[1].lo - e[2].lo - e[3].lo,
                 top(e[0].V) + top(e[1].V) + top(e[2].V) + top(e[3].V), e[0].V + e[1].V + e[2].V + e[3].V);
        break;
    case OP_NEG: r.res = Env{-e[0].hi, -e[0].lo, e[0].V}; break;                 // limb-wise: a strict -2^29 becomes 2^29
    case OP_MUL:
        product_operand(0);
        product_operand(1);
        r.res = Env{STRICT_LO, STRICT_HI, product_v(e[0].V * e[1].V)};
        break;
    case OP_SQR:
        product_operand(0);
        r.res = Env{STRICT_LO, STRICT_HI, product_v(e[0].V * e[0].V)};
        break;
    case OP_DOT2:
        for (int i = 0; i < 4; ++i) product_operand(i);
        if (e[0].V * e[1].V + e[2].V * e[3].V > DOT2_VV) fail(-1, "|a||b| + |c||d| not below 288 p^2");
        r.res = Env{STRICT_LO, STRICT_HI, product_v(e[0].V * e[1].V + e[2].V * e[3].V)};
        break;
    case OP_IS_ZERO_MOD_REDUCED:
    case OP_LIMB0_OF_ZERO_MOD:
        if (e[0].lo < STRICT_LO || e[0].hi > STRICT_HI) fail(0, "limbs not strict");
        if (e[0].V > REDUCED_V) fail(0, "value not in (-2p, 2p)");
        r.res = e[0];
        break;
    case OP_CANONICAL_LT2P:
        if (e[0].V > REDUCED_V) fail(0, "value not in (-2p, 2p)");
        r.res = Env{STRICT_LO, STRICT_HI, VU};                                  // [0, p)
        break;
    case OP_LIMBS_ZERO: r.res = e[0]; break;
    default: fail(-1, "unknown operation");
    }
    return r;
}

// ---- the record of violations
struct Record {
    std::string site;
    int role;             // quad role of the lane that ran the operation; -1 outside ecq.cuh
    int seq;              // the how-manieth checked operation since the site tag was set
    bool escape;          // false: a precondition missed;  true: a concrete result outside the envelope its rule predicts
    int op, operand;
    std::string detail;
};
inline std::mutex& log_mutex() {
    static std::mutex m;
    return m;
}
inline std::vector<Record>& log() {
    static std::vector<Record> l;
    return l;
}
struct Where {
    std::string site = "-";
    int role = -1, seq = 0;
};
inline Where& where() {
    static thread_local Where w;
    return w;
}
inline void set_site(const std::string& s, int role = -1) {
    where().site = s;
    where().role = role;
    where().seq = 0;
}
inline std::string env_text(const Env& e) {
    char b[96];
    snprintf(b, sizeof b, "[%lld, %lld] V=%.4f", (long long)e.lo, (long long)e.hi, (double)e.V / VU);
    return b;
}
inline void record(bool escape, int op, int operand, const char* why, const Env* es, int n) {
    Record r{where().site, where().role, where().seq, escape, op, operand, why};
    for (int i = 0; i < n; ++i) r.detail += std::string(i == operand ? " *" : " ") + (char)('a' + i) + "=" + env_text(es[i]);
    std::lock_guard<std::mutex> g(log_mutex());
    log().push_back(r);
}
inline std::string record_text(const Record& r) {
    char b[64];
    std::string s = r.site + "|role " + std::to_string(r.role) + "|op #" + std::to_string(r.seq) + " " + op_name(r.op) + "|";
    if (r.escape) s += "result outside its envelope";
    else if (r.operand < 0) s += "operands";
    else {
        snprintf(b, sizeof b, "operand %c", 'a' + r.operand);
        s += b;
    }
    return s + "|" + r.detail;
}

// a limb that takes its element's envelope along: ecq.cuh moves elements between lanes limb by limb
struct BLimb {
    uint32_t x;
    Env e;
};

}   // namespace fb

template <class P>
struct Fb {
    typedef Fs<P> S;
    static constexpr int NL = P::NL;
    static constexpr int SAT = P::SAT_WORDS;
    fb::BLimb v[NL];

    // ---- the envelope and the value
    static int64_t tp() { return (int64_t)P::MOD(NL - 1) + 1; }
    // 2^(32 SAT) / p, rounded up: what split_words can return
    static int64_t words_v() { return ((fb::VU << (32 * SAT - 30 * (NL - 1))) + (P::MOD(NL - 1) - 2)) / (P::MOD(NL - 1) - 1); }
    S fs() const {
        S s;
        for (int i = 0; i < NL; ++i) s.v[i] = v[i].x;
        return s;
    }
    fb::Env env() const {
        fb::Env e = v[0].e;
        for (int i = 1; i < NL; ++i) e = fb::join(e, v[i].e);
        return e;
    }
    void set_env(const fb::Env& e) {
        for (int i = 0; i < NL; ++i) v[i].e = e;
    }
    static Fb wrap(const S& s, const fb::Env& e) {
        Fb r;
        for (int i = 0; i < NL; ++i) r.v[i] = fb::BLimb{s.v[i], e};
        return r;
    }
    // are the concrete limbs where the envelope says?  (|value| / p in long double: 64 bits against a bound held to 16)
    static bool concrete_inside(const S& s, const fb::Env& e) {
        long double val = 0, mod = 0;
        bool all_zero = true;
        for (int i = NL - 1; i >= 0; --i) {
            const int32_t x = (int32_t)s.v[i];
            all_zero = all_zero && x == 0;
            if (i < NL - 1 && (x < e.lo || x > e.hi)) return false;
            val = val + (long double)x * __builtin_ldexpl(1.0L, 30 * (i - NL + 1));
            mod = mod + (long double)P::MOD(i) * __builtin_ldexpl(1.0L, 30 * (i - NL + 1));
        }
        if (e.V == 0) return all_zero;
        const long double ratio = (val < 0 ? -val : val) / mod;
        return ratio * fb::VU < (long double)e.V * (1.0L + 1e-12L);
    }
    // check the precondition, record a miss, hand the result its envelope
    static fb::Env checked(int op, const S* result, std::initializer_list<fb::Env> operands) {
        where_next();
        const fb::RuleOut ro = fb::rule(op, operands.begin(), tp(), words_v());
        if (!ro.ok) fb::record(false, op, ro.operand, ro.why, operands.begin(), (int)operands.size());
        if (result && !concrete_inside(*result, ro.res)) fb::record(true, op, -1, "", &ro.res, 1);
        return ro.res;
    }
    static void where_next() { ++fb::where().seq; }
    static Fb out(int op, const S& result, std::initializer_list<fb::Env> operands) { return wrap(result, checked(op, &result, operands)); }

    // ---- the interface XYZZu<F> and ecq.cuh use
    static Fb zero() { return out(fb::OP_ZERO, S::zero(), {}); }
    static Fb one() { return out(fb::OP_ONE, S::one(), {}); }
    static Fb add(const Fb& a, const Fb& b) { return out(fb::OP_ADD, S::add(a.fs(), b.fs()), {a.env(), b.env()}); }
    static Fb dbl(const Fb& a) { return out(fb::OP_DBL, S::dbl(a.fs()), {a.env()}); }
    static Fb add3(const Fb& a, const Fb& b, const Fb& c) { return out(fb::OP_ADD3, S::add3(a.fs(), b.fs(), c.fs()), {a.env(), b.env(), c.env()}); }
    static Fb sub(const Fb& a, const Fb& b) { return out(fb::OP_SUB, S::sub(a.fs(), b.fs()), {a.env(), b.env()}); }
    static Fb sub_sum3(const Fb& a, const Fb& b, const Fb& c, const Fb& d) {
        return out(fb::OP_SUB_SUM3, S::sub_sum3(a.fs(), b.fs(), c.fs(), d.fs()), {a.env(), b.env(), c.env(), d.env()});
    }
    static Fb neg(const Fb& a) { return out(fb::OP_NEG, S::neg(a.fs()), {a.env()}); }
    static Fb mul(const Fb& a, const Fb& b) { return out(fb::OP_MUL, S::mul(a.fs(), b.fs()), {a.env(), b.env()}); }
    static Fb sqr(const Fb& a) { return out(fb::OP_SQR, S::sqr(a.fs()), {a.env()}); }
    static Fb dot2(const Fb& a, const Fb& b, const Fb& c, const Fb& d) {
        return out(fb::OP_DOT2, S::dot2(a.fs(), b.fs(), c.fs(), d.fs()), {a.env(), b.env(), c.env(), d.env()});
    }
    // Fs::inverse is the shared exponentiation loop over Fs::one / sqr / mul: here the same loop runs over the checked operators, so
    // every product inside it is checked; the value is the one Fs::inverse gives
    static Fb inverse(const Fb& a) {
        uint32_t e[SAT];
        for (int i = 0; i < SAT; ++i) e[i] = P::MODW(i);
        zk_words_minus_two(e);
        const Fb r = zk_pow_words(a, e, SAT);
        const S want = S::inverse(a.fs());
        if (memcmp(want.v, r.fs().v, sizeof want.v) != 0) fb::record(true, fb::OP_MUL, -1, "inverse differs from Fs::inverse", nullptr, 0);
        return r;
    }
    bool limbs_zero() const {
        checked(fb::OP_LIMBS_ZERO, nullptr, {env()});
        return fs().limbs_zero();
    }
    bool is_zero_mod_reduced() const {
        checked(fb::OP_IS_ZERO_MOD_REDUCED, nullptr, {env()});
        return fs().is_zero_mod_reduced();
    }
    bool limb0_of_zero_mod() const {
        checked(fb::OP_LIMB0_OF_ZERO_MOD, nullptr, {env()});
        return fs().limb0_of_zero_mod();
    }
    static Fb canonical_lt2p(const Fb& a) { return out(fb::OP_CANONICAL_LT2P, S::canonical_lt2p(a.fs()), {a.env()}); }

    // ---- the way in and out for the harness (fields.cuh from_sat / to_sat, written over the checked product)
    static Fb constant(int32_t (*limb)(int)) {              // a generated constant: balanced digits of a residue in [0, p)
        S s;
        for (int i = 0; i < NL; ++i) s.v[i] = (uint32_t)limb(i);
        return wrap(s, fb::Env{fb::STRICT_LO, fb::STRICT_HI, fb::VU});
    }
    static Fb from_sat(const uint32_t* w) { return mul(out(fb::OP_WORDS, S::split_words(w), {}), constant(P::C_IN)); }
    void to_sat(uint32_t* w) const {
        const Fb m = mul(*this, constant(P::C_OUT));
        checked(fb::OP_CANONICAL_LT2P, nullptr, {m.env()});   // canon_floor: the same (-2p, 2p)
        S::canon_floor(m.fs()).pack_words(w);
    }
};
