// The schedule tables of the table-driven steps (chol.hip's balanced schedule, one_launch.hip's long series, batch_step.hip's
// batched step): built on the host once per shape and kept for the life of the library, with a copy in PINNED host memory
// that volt_*_workspace_init copies into the caller's scratch -- the library owns no device memory.  Host code only.
#pragma once
#include <hip/hip_runtime.h>
#include <array>
#include <map>
#include <mutex>
#include <string.h>
#include <utility>
#include <vector>

namespace volt {

// Plan: what a caller keeps beside the table, plus `std::vector<int4> image` -- the table as it is copied, header included
// (empty: no table for this key).  The plan of a key is built at most once per process, by `build(plan)` under the cache's
// mutex; plan() makes no HIP call, so a size query may use it.  table() adds the pinned copy, per (current device, key):
// made on first need; NOT while `s` is being captured into a graph (no allocation inside a capture) -- that call returns
// "no table" (plan == nullptr) and remembers nothing; a failed allocation IS remembered: no retry per call.
template <class Plan, size_t K>
class TableCache {
public:
    using Key = std::array<int, K>;
    struct Table {
        const Plan* plan = nullptr;              // nullptr: no table
        const int4* pinned = nullptr;            // plan->image, in pinned host memory
    };
    template <class Build>
    const Plan& plan(const Key& key, Build&& build) {
        std::lock_guard<std::mutex> lock(mu);
        return find_or_build(key, build);
    }
    template <class Build>
    Table table(const Key& key, hipStream_t s, Build&& build) {
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess) return Table();
        std::lock_guard<std::mutex> lock(mu);
        auto it = tables.find({dev, key});
        if (it != tables.end()) return it->second;
        hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
        if (hipStreamIsCapturing(s, &cap) != hipSuccess || cap != hipStreamCaptureStatusNone) return Table();
        const Plan& pl = find_or_build(key, build);
        const size_t bytes = pl.image.size() * sizeof(int4);
        int4* pinned = nullptr;
        if (bytes && hipHostMalloc((void**)&pinned, bytes, hipHostMallocDefault) != hipSuccess) {
            (void)hipGetLastError();
            pinned = nullptr;
        }
        if (pinned) memcpy(pinned, pl.image.data(), bytes);
        return tables[{dev, key}] = pinned ? Table{&pl, pinned} : Table();   // a failure is remembered too
    }

private:
    template <class Build>
    const Plan& find_or_build(const Key& key, Build&& build) {
        auto it = plans.find(key);
        if (it == plans.end()) {
            it = plans.emplace(key, Plan()).first;
            build(it->second);
        }
        return it->second;
    }
    std::mutex mu;
    std::map<Key, Plan> plans;                                   // (a map's elements never move: the pointers handed out stay good)
    std::map<std::pair<int, Key>, Table> tables;
};

// the install step of a workspace: the pinned table into the caller's region
inline int install_table(void* dst, const int4* pinned, size_t bytes, hipStream_t s) {
    hipError_t e = hipMemcpyAsync(dst, pinned, bytes, hipMemcpyHostToDevice, s);
    return e != hipSuccess ? (int)e : 0;
}

}  // namespace volt
