// The library's process-wide state (host code only, no kernel): the tuning table after the environment and the device's
// topology, and the per-device stream pool.  Declared in host.h.
#include "host.h"
#include "../../include/volt_hip.h"
#include "../../include/volt_hip_tune.h"
#include <mutex>
#include <stdlib.h>

static Tunables read_env(Tunables t) {                       // VOLT_TUNE=1 processes only
    auto geti = [](const char* name, int& v) { if (const char* e = getenv(name)) v = atoi(e); };
        geti("VOLT_GROUPS", t.groups);
        geti("VOLT_SPLITK_TARGET", t.splitk_target);
        geti("VOLT_SPLITK_MINL", t.splitk_minl);
        geti("VOLT_SPLITK_MAXS", t.splitk_maxs);
        geti("VOLT_SPLITK_GROUPS", t.splitk_groups);
        geti("VOLT_SPLITK_MAXB", t.splitk_maxb);
        geti("VOLT_SCHED", t.sched);
        geti("VOLT_SCHED_MINB", t.sched_minb);
        geti("VOLT_SCHED_MAXB", t.sched_maxb);
        geti("VOLT_SCHED_MAXB_POTRF", t.sched_maxb_potrf);
        geti("VOLT_SCHED_G", t.sched_g);
        geti("VOLT_SCHED_S", t.sched_s);
        geti("VOLT_SCHED_GROUPS", t.sched_groups);
        geti("VOLT_SCHED_KMIN", t.sched_kmin);
        geti("VOLT_SMALL_NMAX", t.small_nmax);
        geti("VOLT_SMALL_MAXWG", t.small_maxwg);
        geti("VOLT_SMALL_PAD_MAXB", t.small_pad_maxb);
        geti("VOLT_SMALL_MAXB", t.small_maxb);
        geti("VOLT_SMALL_MAXB2", t.small_maxb2);
        geti("VOLT_LONG", t.long_on);
        geti("VOLT_LONG_FIRST", t.long_first);
        geti("VOLT_LONG_EMIN", t.long_emin);
        geti("VOLT_LONG_PAD", t.long_pad);
        geti("VOLT_LONG_NMIN", t.long_nmin);
        geti("VOLT_LONG_XCD", t.long_xcd);
        geti("VOLT_LONG_SPLIT", t.long_split);
        geti("VOLT_PLAIN_SPREAD", t.plain_spread);
        geti("VOLT_SPLIT_SPREAD", t.split_spread);
        geti("VOLT_BATCH", t.batch);
        geti("VOLT_BATCH_ORDER", t.batch_order);
        geti("VOLT_BATCH_LOCAL", t.batch_local);
        geti("VOLT_BATCH_SPREAD", t.batch_spread);
        geti("VOLT_BATCH_LAD", t.batch_lad);
        geti("VOLT_BATCH_PULLERS", t.batch_pullers);
        geti("VOLT_ROLLOUT_LANE", t.rollout_lane);
        geti("VOLT_LONG_PULLERS", t.long_pullers);
        geti("VOLT_BATCH_XSKEW", t.batch_xskew);
        geti("VOLT_BATCH_XDROP", t.batch_xdrop);
        geti("VOLT_BATCH64", t.batch64);
        geti("VOLT_BATCH64_MAX", t.batch64_max);
        geti("VOLT_BATCH64_MAX_STEP", t.batch64_max_step);
        geti("VOLT_F64_LOOKAHEAD", t.f64_lookahead);
        geti("VOLT_F64_TRTRI_LOOKAHEAD", t.f64_trtri_lookahead);
        geti("VOLT_F64_SPREAD", t.f64_spread);
        geti("VOLT_F64_SPLIT_TARGET", t.f64_split_target);
        if (const char* e = getenv("VOLT_SCHED_FRAC")) t.sched_frac = (float)atof(e);
        geti("VOLT_FAKE_CUS", t.cus);                        // tests: plan as if the device had this many CUs / XCDs
        geti("VOLT_FAKE_XCCS", t.xccs);
    return t;
}

// What the device looks like, and the gates that depend on it (host.h).  A process without a device (the CPU-side tests)
// keeps the full-chip defaults.
static void apply_topology(Tunables& t, bool faked) {
    if (!faked) {
        int dev = 0, cus = 0, xccs = 0;
        if (hipGetDevice(&dev) == hipSuccess &&
            hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && cus > 0) {
            t.cus = cus;
            if (hipDeviceGetAttribute(&xccs, hipDeviceAttributeNumberOfXccs, dev) == hipSuccess && xccs > 0) t.xccs = xccs;
        } else {
            (void)hipGetLastError();
        }
    }
    if (t.cus == 256 && t.xccs == 8) return;
    const double f = t.cus / 256.0;
    auto scale = [f](int v, int lo) { const int r = (int)(v * f + 0.5); return r < lo ? lo : r; };
    t.sched_g = scale(t.sched_g, 8);
    t.plain_spread = scale(t.plain_spread, 8);
    t.split_spread = scale(t.split_spread, 16);
    t.splitk_target = scale(t.splitk_target, 16);
    t.group_gate = scale(t.group_gate, 16);
    t.batch_spread = scale(t.batch_spread, 8);
    t.small_nmax = 0;                                        // the one-launch steps: tuned for, and (batched step) placed on, the full chip
    t.long_on = 0;
    t.batch = 0;
    t.batch64 = 0;
}

const Tunables& tunables() {
    static const Tunables tn = [] {
        const char* tune0 = getenv("VOLT_TUNE");
        const bool tuning = tune0 && atoi(tune0) != 0;
        const bool faked = tuning && (getenv("VOLT_FAKE_CUS") || getenv("VOLT_FAKE_XCCS"));
        Tunables t = [&] {
            Tunables t;
            if (!tuning) return t;                           // the frozen defaults
            return read_env(t);
        }();
        apply_topology(t, faked);
        return t;
    }();
    return tn;
}

// The auxiliary streams and the fork / join events of a device, created once (library-lifetime, like a BLAS handle's):
// chol.hip's stream groups (run_factor_groups, where the scheme is described) and chol64.hip's look-ahead schedules run on
// them, under the pool's mutex while they enqueue.
StreamPool* stream_pool() {
    static StreamPool pools[16];
    static std::once_flag once[16];
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 16) return nullptr;
    // (lowest-priority streams for the bulk work were tried: the chain then waits for events from a stream the hardware
    // serves last -- one 4096^2 matrix 4.2 -> 8.1 ms)
    std::call_once(once[dev], [dev]() {
        StreamPool& p = pools[dev];
        bool ok = hipEventCreateWithFlags(&p.fork, hipEventDisableTiming) == hipSuccess;
        for (int i = 0; i < MAX_GROUPS - 1; ++i) {
            ok = ok && hipStreamCreateWithFlags(&p.aux[i], hipStreamNonBlocking) == hipSuccess;
            ok = ok && hipEventCreateWithFlags(&p.join[i], hipEventDisableTiming) == hipSuccess;
        }
        for (int i = 0; i < 5; ++i) ok = ok && hipEventCreateWithFlags(&p.extra[i], hipEventDisableTiming) == hipSuccess;
        p.want_groups = tunables().groups;
        if (p.want_groups < 1) p.want_groups = 1;
        if (p.want_groups > MAX_GROUPS) p.want_groups = MAX_GROUPS;
        p.ok = ok;
    });
    return pools[dev].ok ? &pools[dev] : nullptr;
}

extern "C" {

// What the library found the device to be, and the gates that follow from it (host.h): out[0] CUs, [1] XCDs, [2] slots the
// balanced schedule plans for, [3] / [4] plain / split launches up to this many workgroups run one per CU, [5] launches
// below this many workgroups run as one stream group, [6] one-launch steps enabled (short series | one long series << 1 |
// batched << 2).  No GPU needed (a process without a device reports the full-chip defaults).
int volt_topology_describe(int* out) {
    if (!out) return -1;
    const Tunables& tn = tunables();
    out[0] = tn.cus;
    out[1] = tn.xccs;
    out[2] = tn.sched_g;
    out[3] = tn.plain_spread;
    out[4] = tn.split_spread;
    out[5] = tn.group_gate;
    out[6] = (tn.small_nmax > 0 ? 1 : 0) | (tn.long_on ? 2 : 0) | (tn.batch > 0 ? 4 : 0);
    return 0;
}

}  // extern "C"
