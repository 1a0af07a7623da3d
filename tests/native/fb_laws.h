// Closure of the G1 group law under the contract of fields.cuh: XYZZu<F> (ecu.cuh) and qadd / qdbl (ecq.cuh, unmodified) instantiated
// over the checked field Fb (fb_field.h).  Every function is run once per branch outcome on a concrete input that takes the branch,
// with the envelopes of its inputs widened to the class invariant below; it must record no violation and return envelopes inside
// the same invariant.  Envelopes do not depend on values, so this is the induction step: any chain of these functions stays inside
// the contract for every input.
#pragma once
#include <condition_variable>
#include <functional>
#include <thread>
#include "fb_field.h"

// ---- the five wave primitives ecq.cuh uses, for host threads that run in lockstep (one thread per lane, a barrier around each
// exchange).  Declared before ecq.cuh is read: its templates name them unqualified.
namespace wave {
struct Ctx {
    int lanes = 0, waiting = 0;
    uint64_t generation = 0;
    std::mutex m;
    std::condition_variable cv;
    unsigned char slot[64][64];
    void sync() {
        std::unique_lock<std::mutex> g(m);
        const uint64_t gen = generation;
        if (++waiting == lanes) {
            waiting = 0;
            ++generation;
            cv.notify_all();
        } else {
            cv.wait(g, [&] { return generation != gen; });
        }
    }
};
inline Ctx*& ctx() {
    static thread_local Ctx* c = nullptr;
    return c;
}
inline int& lane() {
    static thread_local int l = 0;
    return l;
}
template <class T>
T exchange(const T& mine, int src) {
    static_assert(sizeof(T) <= 64, "slot too small");
    Ctx* c = ctx();
    memcpy(c->slot[lane()], &mine, sizeof(T));
    c->sync();
    T r;
    memcpy(&r, c->slot[src], sizeof(T));
    c->sync();
    return r;
}
// run fn(lane) on `lanes` threads that share one wave
inline void run(int lanes, const std::function<void(int)>& fn) {
    Ctx c;
    c.lanes = lanes;
    std::vector<std::thread> t;
    for (int l = 0; l < lanes; ++l)
        t.emplace_back([&c, &fn, l] {
            ctx() = &c;
            lane() = l;
            fn(l);
        });
    for (auto& th : t) th.join();
}
}   // namespace wave
template <class T>
inline T __shfl(const T& v, int src, int) { return wave::exchange(v, src); }
template <class T>
inline T __shfl_xor(const T& v, int mask, int) { return wave::exchange(v, wave::lane() ^ mask); }
inline unsigned __lane_id() { return (unsigned)wave::lane(); }
inline unsigned long long __ballot(bool f) {
    wave::Ctx* c = wave::ctx();
    c->slot[wave::lane()][0] = f ? 1 : 0;
    c->sync();
    unsigned long long b = 0;
    for (int l = 0; l < c->lanes; ++l) b |= (unsigned long long)c->slot[l][0] << l;
    c->sync();
    return b;
}
inline bool __any(bool f) { return __ballot(f) != 0; }

#include "../../ark_plonk_amd/csrc/ecq.cuh"

namespace fbl {
using fb::Env;

// ---- the class invariant (DESIGN.md "Signed-limb contract of the G1 law"; ecu.cuh header; what the kernels store)
inline Env inv_x() { return Env{-fb::ALMOST, fb::ALMOST, 4 * fb::VU}; }                // ecu.cuh: stored |X| < 4p, a sum of four products
inline Env inv_y() { return Env{-(1ll << 29), 1ll << 29, fb::VU}; }                    // a product, or its limb-wise negation (XYZZu::neg, msm_accumulate.hip)
inline Env inv_zz() { return Env{fb::STRICT_LO, fb::STRICT_HI, fb::VU}; }              // ZZ, ZZZ: products
inline Env inv_ax() { return inv_zz(); }                                               // affine x: strict, (-p, p)
inline Env inv_ay() { return inv_y(); }                                                // affine y: may be negated limb-wise
inline Env inv_role(int role) { return role == 0 ? inv_x() : role == 1 ? inv_y() : inv_zz(); }

template <class P>
struct Closure {
    typedef Fb<P> F;
    typedef Fs<P> S;
    typedef XYZZu<F> X;
    typedef AffineU<F> A;
    std::string report;
    int failures = 0;
    size_t mark = 0;
    std::string name;

    void fail(const std::string& why) {
        ++failures;
        report += "FAIL " + name + ": " + why + "\n";
    }
    void begin(const std::string& n) {
        name = n;
        fb::set_site(n);
        std::lock_guard<std::mutex> g(fb::log_mutex());
        mark = fb::log().size();
    }
    // every record since begin() is a failure of this case
    void end() {
        std::lock_guard<std::mutex> g(fb::log_mutex());
        for (size_t i = mark; i < fb::log().size(); ++i) {
            ++failures;
            report += "VIOLATION " + fb::record_text(fb::log()[i]) + "\n";
        }
        report += "CASE " + name + "\n";
        fb::set_site("-");
    }
    void need_inside(const char* what, const F& f, const Env& inv) {
        if (!fb::inside(f.env(), inv)) fail(std::string(what) + " leaves the invariant: " + fb::env_text(f.env()) + " against " + fb::env_text(inv));
    }
    void out_xyzz(const X& p) {
        need_inside("X", p.x, inv_x());
        need_inside("Y", p.y, inv_y());
        need_inside("ZZ", p.zz, inv_zz());
        need_inside("ZZZ", p.zzz, inv_zz());
    }
    void out_affine(const A& a) {
        need_inside("x", a.x, inv_ax());
        need_inside("y", a.y, inv_ay());
    }
    // an input: the concrete value must be a member of the class, then its envelope is widened to the whole class
    F widen(const F& f, const Env& inv) {
        if (!fb::inside(f.env(), inv)) fail("an input of the case is outside the invariant: " + fb::env_text(f.env()));
        F r = f;
        r.set_env(inv);
        return r;
    }
    X widen(const X& p) {
        X r;
        r.x = widen(p.x, inv_x());
        r.y = widen(p.y, inv_y());
        r.zz = widen(p.zz, inv_zz());
        r.zzz = widen(p.zzz, inv_zz());
        return r;
    }
    A widen(const A& a) {
        A r;
        r.x = widen(a.x, inv_ax());
        r.y = widen(a.y, inv_ay());
        return r;
    }

    // the group element, for "did the case take the branch it names": canonical affine words over the unchecked field
    static XYZZu<S> strip(const X& p) {
        XYZZu<S> r;
        r.x = p.x.fs();
        r.y = p.y.fs();
        r.zz = p.zz.fs();
        r.zzz = p.zzz.fs();
        return r;
    }
    static bool same_point(const XYZZu<S>& a, const XYZZu<S>& b) {
        AffineU<S> u, w;
        const bool fa = a.to_affine(u), fb_ = b.to_affine(w);
        if (fa != fb_) return false;
        if (!fa) return true;
        uint32_t ux[S::SAT], uy[S::SAT], wx[S::SAT], wy[S::SAT];
        u.x.to_sat(ux);
        u.y.to_sat(uy);
        w.x.to_sat(wx);
        w.y.to_sat(wy);
        return memcmp(ux, wx, sizeof ux) == 0 && memcmp(uy, wy, sizeof uy) == 0;
    }
    void want(const X& got, const XYZZu<S>& expect) {
        if (!same_point(strip(got), expect)) fail("not the group element the branch gives");
    }

    // the concrete points of the cases, from two affine points P, Q (Q != +-P, neither of order 2 or 3):
    A aP, aQ, a2P, a2Pn;      // P, Q, 2P in affine form and -(2P)
    X x2P, x2Q, x2Pu, inf;    // 2P and 2Q with ZZ != 1; 2P with ZZ = 1
    void setup(const uint32_t* words) {
        fb::set_site("setup");
        const int W = S::SAT;
        aP.x = F::canonical_lt2p(F::from_sat(words));
        aP.y = F::canonical_lt2p(F::from_sat(words + W));
        aQ.x = F::canonical_lt2p(F::from_sat(words + 2 * W));
        aQ.y = F::canonical_lt2p(F::from_sat(words + 3 * W));
        x2P = X::dbl_affine(aP);
        x2Q = X::dbl_affine(aQ);
        A t;
        x2P.to_affine(t);
        a2P.x = F::canonical_lt2p(t.x);      // stored affine coordinates are canonical
        a2P.y = F::canonical_lt2p(t.y);
        a2Pn = a2P;
        a2Pn.y = F::neg(a2P.y);
        x2Pu = X::from_affine(a2P);
        inf = X::infinity();
    }

    void single_lane() {
        const XYZZu<S> e2P = strip(x2P), eInf = XYZZu<S>::infinity();
        const XYZZu<S> e4P = XYZZu<S>::dbl(e2P);
        const XYZZu<S> e2P2Q = XYZZu<S>::add(e2P, strip(x2Q));
        const XYZZu<S> e2PQ = XYZZu<S>::add(e2P, XYZZu<S>::from_affine(AffineU<S>{aQ.x.fs(), aQ.y.fs()}));
        X r;
        A a;

        begin("from_affine");
        a = widen(aP);
        r = X::from_affine(a);
        out_xyzz(r);
        end();

        begin("dbl_affine");
        a = widen(aP);
        r = X::dbl_affine(a);
        out_xyzz(r);
        want(r, e2P);
        end();

        begin("dbl/infinity");
        r = X::dbl(widen(inf));
        out_xyzz(r);
        want(r, eInf);
        end();
        begin("dbl/general");
        r = X::dbl(widen(x2P));
        out_xyzz(r);
        want(r, e4P);
        end();

        begin("madd/p infinite");
        r = X::madd(widen(inf), widen(a2P));
        out_xyzz(r);
        want(r, e2P);
        end();
        begin("madd/P = Q");
        r = X::madd(widen(x2P), widen(a2P));
        out_xyzz(r);
        want(r, e4P);
        end();
        begin("madd/P = -Q");
        r = X::madd(widen(x2P), widen(a2Pn));
        out_xyzz(r);
        want(r, eInf);
        end();
        begin("madd/general");
        r = X::madd(widen(x2P), widen(aQ));
        out_xyzz(r);
        want(r, e2PQ);
        end();

        struct Half {
            const char* name;
            const A* q;
            int how;
        } halves[3] = {{"madd_begin + madd_finish/general", &aQ, X::MADD_SUM},
                       {"madd_begin + madd_finish/P = Q", &a2P, X::MADD_SAME},
                       {"madd_begin + madd_finish/P = -Q", &a2Pn, X::MADD_OPPOSITE}};
        for (const Half& h : halves) {
            begin(h.name);
            X p = widen(x2P);
            const typename X::MaddHalf mh = X::madd_begin(p, widen(*h.q));
            const int how = X::madd_finish(p, mh);
            if (how != h.how) fail("madd_finish returned " + std::to_string(how));
            if (how == X::MADD_SUM) {            // otherwise p is left undefined: the caller does not read it
                out_xyzz(p);
                want(p, e2PQ);
            }
            end();
        }

        begin("add/p infinite");
        r = X::add(widen(inf), widen(x2P));
        out_xyzz(r);
        want(r, e2P);
        end();
        begin("add/q infinite");
        r = X::add(widen(x2P), widen(inf));
        out_xyzz(r);
        want(r, e2P);
        end();
        begin("add/P = Q");
        r = X::add(widen(x2P), widen(x2Pu));
        out_xyzz(r);
        want(r, e4P);
        end();
        begin("add/P = -Q");
        r = X::add(widen(x2P), widen(X::neg(x2Pu)));
        out_xyzz(r);
        want(r, eInf);
        end();
        begin("add/general");
        r = X::add(widen(x2P), widen(x2Q));
        out_xyzz(r);
        want(r, e2P2Q);
        end();

        begin("neg");
        r = X::neg(widen(x2P));
        out_xyzz(r);
        want(X::neg(r), e2P);
        end();

        begin("to_affine/infinity");
        if (widen(inf).to_affine(a)) fail("infinity came out finite");
        out_affine(a);
        end();
        begin("to_affine/general");
        if (!widen(x2P).to_affine(a)) fail("a finite point came out as infinity");
        out_affine(a);
        want(X::from_affine(a), e2P);
        end();
        // the normalisation from a known 1 / ZZZ (the key fold of ipa.hip).  i3 is a product at every call site: a Fermat power, or
        // the product of one with the prefix and suffix products of block_inverse.cuh
        begin("to_affine_given");
        {
            const F i3 = widen(F::inverse(x2P.zzz), inv_zz());
            widen(x2P).to_affine_given(i3, a);
            out_affine(a);
            want(X::from_affine(a), e2P);
        }
        end();
    }

    // ---- ecq.cuh: one quad per case, every case of a call in one wave (so every lane runs the P = +-Q path as well), four lanes each
    struct QuadCase {
        std::string name;
        X p, q;
        XYZZu<S> expect;
    };
    static F coord(const X& p, int role) { return quad_pick(p, (uint32_t)role); }
    void run_quads(const char* fn, bool is_add, const std::vector<QuadCase>& cases) {
        const int lanes = 4 * (int)cases.size();
        std::vector<F> res(lanes);
        std::vector<X> pw, qw;
        begin(std::string(fn) + "/inputs");
        for (const QuadCase& c : cases) {
            pw.push_back(widen(c.p));
            qw.push_back(widen(c.q));
        }
        end();
        size_t from;
        {
            std::lock_guard<std::mutex> g(fb::log_mutex());
            from = fb::log().size();
        }
        wave::run(lanes, [&](int lane) {
            const int role = lane & 3;
            const QuadCase& c = cases[lane >> 2];
            fb::set_site(std::string(fn) + "/" + c.name, role);
            const F p = coord(pw[lane >> 2], role), q = coord(qw[lane >> 2], role);
            res[lane] = is_add ? qadd<F>(p, q, (uint32_t)role) : qdbl<F>(p, (uint32_t)role);
        });
        for (size_t k = 0; k < cases.size(); ++k) {
            name = std::string(fn) + "/" + cases[k].name;
            X got;
            got.x = res[4 * k];
            got.y = res[4 * k + 1];
            got.zz = res[4 * k + 2];
            got.zzz = res[4 * k + 3];
            for (int role = 0; role < 4; ++role) {
                const std::string what = "role " + std::to_string(role);
                need_inside(what.c_str(), res[4 * k + role], inv_role(role));
            }
            want(got, cases[k].expect);
            report += "CASE " + name + "\n";
        }
        // what the lanes recorded goes out as it is: the test holds the list of dead-lane entries and exempts exactly those
        std::lock_guard<std::mutex> g(fb::log_mutex());
        for (size_t i = from; i < fb::log().size(); ++i) report += "QUADVIOLATION " + fb::record_text(fb::log()[i]) + "\n";
    }
    void quad() {
        const XYZZu<S> e2P = strip(x2P), e2Q = strip(x2Q), eInf = XYZZu<S>::infinity();
        const XYZZu<S> e4P = XYZZu<S>::dbl(e2P), e2P2Q = XYZZu<S>::add(e2P, e2Q);
        const std::vector<QuadCase> adds = {
            {"general", x2P, x2Q, e2P2Q},   {"P = Q", x2P, x2Pu, e4P},   {"P = -Q", x2P, X::neg(x2Pu), eInf},
            {"p infinite", inf, x2Q, e2Q},  {"q infinite", x2P, inf, e2P}, {"both infinite", inf, inf, eInf},
        };
        run_quads("qadd", true, adds);
        run_quads("qadd alone", true, {adds[0]});      // no lane of the wave is slow: the branch around qdbl is walked past
        run_quads("qdbl", false, {{"general", x2P, inf, e4P}, {"infinity", inf, inf, eInf}});
    }
};

template <class P>
int closure(int which, const uint32_t* words, char* out, int cap) {
    {
        std::lock_guard<std::mutex> g(fb::log_mutex());
        fb::log().clear();
    }
    Closure<P> c;
    c.begin("setup");
    c.setup(words);
    c.end();
    if (which == 0) c.single_lane();
    else c.quad();
    snprintf(out, (size_t)cap, "%s", c.report.c_str());
    return c.failures;
}
}   // namespace fbl
