// tn_api_common.h -- what the three C-ABI translation units (tn_api.hip, tn_api_tracer.hip, tn_api_mlp.hip) share.
#pragma once
#include <cstdlib>

#include "../../include/tetranerf_hip.h"
#include "tn_common.h"

namespace tn {

// body of every entry point: 0 and an empty tn_last_error, or 1 and the exception's text
template <typename Fn>
int guarded(Fn &&fn) {
    try {
        fn();
        set_error("");
        return 0;
    } catch (const std::exception &e) {
        set_error(e.what());
        return 1;
    } catch (...) {
        set_error("unknown error");
        return 1;
    }
}

struct DeviceGuard {
    int prev = 0;
    explicit DeviceGuard(int dev) {
        TN_HIP(hipGetDevice(&prev));
        if (prev != dev) TN_HIP(hipSetDevice(dev));
        cur = dev;
    }
    ~DeviceGuard() {
        if (prev != cur) (void)hipSetDevice(prev);
    }
    int cur;
};

inline bool env_flag(const char *name, bool dflt) {
    const char *v = std::getenv(name);
    if (!v || !*v) return dflt;
    return !(v[0] == '0' || v[0] == 'n' || v[0] == 'N' || v[0] == 'f' || v[0] == 'F');
}

// argument checks several entry points share (the messages are the reference's own wording; tests match on them)
inline void check_pow2_M(uint32_t M) {
    if (M == 0 || (M & (M - 1)) != 0) throw Error("max_ray_triangles must be a power of 2.");
}
inline void check_loaded(bool loaded) {
    if (!loaded) throw Error("load_tetrahedra must be called first");
}

}  // namespace tn
