// The per-curve MSM objects (the msm_* units built with -DZK_CURVE_SEL=0/1: msm_common.cuh) export one table of entry points each.
#include "ctx.h"

extern const MsmOps msm_ops_c0, msm_ops_c1;

namespace {
// converts to any MsmOps member: a function that ignores its arguments and returns V
template <int V>
struct Unknown {
    template <class R, class... P>
    using Fn = R (*)(P...);
    template <class R, class... P>
    operator Fn<R, P...>() const {
        return [](P...) -> R { return (R)V; };
    }
};
constexpr Unknown<ZK_ERR_BAD_ARG> bad;
constexpr Unknown<0> zero;
// what an unknown curve id gets, member by member as MsmOps declares them
const MsmOps msm_ops_unknown = {bad, bad, bad, bad, bad, bad, bad, bad, /* partial_dev_supported */ zero, /* partial_dev_bytes */ zero,
                                bad, bad, bad, /* point_bytes */ zero, bad, bad};

const MsmOps* ops_of(CurveBls) { return &msm_ops_c0; }
const MsmOps* ops_of(CurveBn) { return &msm_ops_c1; }
}  // namespace

const MsmOps* msm_ops(int curve) {
    return zk_on_curve(curve, &msm_ops_unknown, [](auto cv) { return ops_of(cv); });
}
