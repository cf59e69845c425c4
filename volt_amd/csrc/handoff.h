// How one workgroup hands data to another workgroup of the SAME launch, how long a waiter waits, and what it reports when it
// gives up.  Every chained kernel of the library (trsv.hip, chol.hip's W_k hand-off, one_launch.hip, batch_step.hip,
// batch64_step.hip, the diagonal-block bodies of tiles.h / tiles64.h) speaks this protocol and no other.
//
// THE WORD.  A hand-off is one 32-bit word per thing handed on: a flag (non-zero, or EQUAL to the number of the step that
// set it -- words that are never cleared: small_step_kernel) or a progress count (>= the number of blocks that are
// complete).  The producer stores its data, makes it visible, then stores the word; a consumer polls the word, then reads.
//
// THE POLL is an sc1 load (relaxed, agent scope): past this CU's L1, served by the XCD's L2 -- or by memory when the line was
// dropped there by a written-through store.  (A scalar poll -- s_load_dword glc, served by the L2 without queueing behind the
// co-resident tile's vector loads -- was measured too: no faster at 64 matrices, 12 % slower at 8, where tiles spin on their
// inputs: 3.73 -> 4.18 ms.)  One lane or one wave polls; a barrier, where the workgroup needs one, covers the rest.
//
// MAKING THE DATA VISIBLE, three ways (Guideline 16 of cdna_hip_programming.md is the first):
//   * plain stores: every storing wave drains (s_waitcnt vmcnt(0)), a barrier, ONE thread issues an agent-scope release
//     (an L2 write-back) and stores the word; the consumer issues one agent-scope acquire (buffer_inv sc1: 1.7 us and more
//     per wave that issues it, MI355X_MICROARCH.md) behind its poll.                                publish_release<false>
//   * WRITTEN-THROUGH stores (sc1: agent-scope relaxed atomic stores, or buffer stores with AUX_SC1; never nt on a
//     hand-off): every storing wave drains, a barrier, the word -- nothing is left in L2 to write back, so NO release; the
//     consumer fetches with sc1 loads and needs no acquire.  This took the L2 write-back and the L2 / L1 invalidate off
//     every hop of a chain (trsv, 8 x 4096 fp32: 4.1 -> 3.0 us per hop; fp64 7.4 -> 6.2; 64 x 2048 0.194 -> 0.139 ms per
//     solve, scripts/bench_trsv.py) and the per-slice releases off the pivot chains.                       publish_wt<false>
//   * LOCALP, the template switch of the waits and publishes below: the writer of everything handed on is known to sit on
//     the SAME XCD as the reader (the batched steps with a batch that is a multiple of 8: the puller queues at the end of
//     this file) and every address handed on is written ONCE per launch, before anything in the launch reads it.  The
//     XCD's L2 is then the point of coherence and no line of the data can be stale in the reader's L1 (invalidated at
//     kernel start, never filled since): the publish is the drain alone and a plain store of the word (which keeps its
//     line in that L2 for the polls), and the waits carry NO acquire fence.  An address that IS written twice per launch
//     takes a real acquire even there (batch64_step.hip, KB = 0).
//
// HOW LONG.  Every wait is bounded by WALL CLOCK (s_memrealtime: a constant 100 MHz counter), not by an iteration count:
// a preempted or profiled run spins more often, not longer.  3 s -- only a bug or a wedged device gets there.  spin_until
// below is the one loop that implements it.
//
// GIVING UP.  A waiter that timed out goes on (it never hangs the device) and reports INFO_HANDOFF_TIMEOUT in the matrix's
// info word, unless a pivot failure is already recorded there; the solves poison their output with NaN and raise their
// error word instead (trsv.hip).  The host treats info <= INT_MIN + 255 as an internal error (include/volt_hip.h).
//
// WHO MAY WAIT FOR WHOM.  A waiter only ever waits for work that is running or finished.  Pieces are handed out by atomic
// tickets in dependency order (trsv.hip, long_step_kernel, the puller queues at the end of this file): no co-residency or
// dispatch-order assumption.  small_step_kernel alone leans on workgroups being dispatched in grid order (one_launch.hip).
#pragma once
#include <hip/hip_runtime.h>

namespace volt {

// ---- what a kernel reports in `info` when it is not a pivot index (include/volt_hip.h) --------------------------------------
constexpr int INFO_HANDOFF_TIMEOUT = -2147483647 - 1;      // INT_MIN: a hand-off timed out
constexpr int INFO_BAD_WORKSPACE = -2147483647;            // INT_MIN + 1: the workspace does not hold what its init wrote
__device__ __forceinline__ void report_timeout(int* info_b) { atomicCAS(info_b, 0, INFO_HANDOFF_TIMEOUT); }

// ---- the bounded spin ------------------------------------------------------------------------------------------------------
#ifndef VOLT_WAIT_TICKS
#define VOLT_WAIT_TICKS 300000000ull                       // 3 s of the 100 MHz s_memrealtime counter
#endif
// the pause between two polls (spins = polls that have failed so far)
struct Pause2 { __device__ __forceinline__ void operator()(unsigned) const { __builtin_amdgcn_s_sleep(2); } };
struct Pause4 { __device__ __forceinline__ void operator()(unsigned) const { __builtin_amdgcn_s_sleep(4); } };
struct PauseBackoff {                                      // a growing pause: the short-series step (one_launch.hip)
    __device__ __forceinline__ void operator()(unsigned spins) const {
        if (spins < 16) __builtin_amdgcn_s_sleep(2);
        else if (spins < 64) __builtin_amdgcn_s_sleep(8);
        else __builtin_amdgcn_s_sleep(24);
    }
};
// Polls done() until it holds; false after VOLT_WAIT_TICKS of wall clock (looked at every 1024th spin).  THE loop: no other
// code of the library reads the clock for a time-out.
template <class Pause = Pause2, class Done>
__device__ __forceinline__ bool spin_until(Done done) {
    if (done()) return true;
    const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
    unsigned spins = 0;
    while (!done()) {
        Pause()(spins);
        if ((++spins & 1023u) == 0 && __builtin_amdgcn_s_memrealtime() - t0 > VOLT_WAIT_TICKS) return false;
    }
    return true;
}

// ---- waits of one lane (or of every lane of a wave, on wave-uniform addresses) ------------------------------------------------
__device__ __forceinline__ int poll_word(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
template <bool LOCALP>
__device__ __forceinline__ void acquire_unless_local() {
    if constexpr (!LOCALP) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    else asm volatile("" ::: "memory");                      // (the compiler keeps later loads behind the poll all the same)
}
// what a word is compared with: IsSet -- `want` = 0: the word is non-zero; else the word EQUALS `want`;  AtLeast -- word >= want
struct IsSet { __device__ __forceinline__ bool operator()(int v, int want) const { return want ? v == want : v != 0; } };
struct AtLeast { __device__ __forceinline__ bool operator()(int v, int want) const { return v >= want; } };
template <class Cmp, class Pause = Pause2>
__device__ __forceinline__ bool wait_word(const int* p, int want) {
    return spin_until<Pause>([&] { return Cmp()(poll_word(p), want); });
}

// The four flags of a diagonal block's column slabs (tiles.h, diag_body<.., SLABS>) sit in one aligned 16-byte word and go up
// in order: ONE load tells how many of them are up, so a tile that arrives late polls once, not once per slab (every poll is a
// round trip on the chain).  Returns how many leading flags equal `want` once that is more than j; -1 on a time-out.
constexpr int AUX_SC1 = 16;                                // aux bits of a buffer load / store: sc1, agent scope
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ int wait_slab_flags(const int* slab, int j, int want) {
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void*)slab, 0, 16, 0x00020000);
    auto count = [&]() {
        asm volatile("" ::: "memory");
        const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(rs, 0, 0, AUX_SC1);
        int c = 0;
        if ((int)v[0] == want) {
            c = 1;
            if ((int)v[1] == want) {
                c = 2;
                if ((int)v[2] == want) c = (int)v[3] == want ? 4 : 3;
            }
        }
        return c;
    };
    int c = 0;
    return spin_until([&] { return (c = count()) > j; }) ? c : -1;
}

// ---- chasing tiles (batch_step.hip, batch64_step.hip: the whole batched step in ONE launch) -----------------------------------
// A left-looking tile reads K blocks 0 .. k-1 of two block rows that other workgroups of the SAME launch are still
// producing.  Instead of waiting for all of them before it starts, a chasing tile follows two progress words ("blocks
// [0, *p - base) of this operand are complete") and asks only at the top of a 128-wide K segment, for the segment whose
// loads it is about to issue -- so the long products run as far ahead as their inputs allow and what is left on the
// critical path behind a finished block column is ONE K block, as in a right-looking sweep, with the left-looking
// traffic.  Every wave polls for itself (the chunk barriers keep the waves of a workgroup within a chunk of each other,
// and each has seen for itself that what it loads is there); a tile that finds everything complete on entry -- the
// common case in a large batch -- never polls again.
struct Chase {
    const int* p0 = nullptr;     // progress word of the X operand's source
    const int* p1 = nullptr;     // ... of the Z operand's
    int base0 = 0, base1 = 0;    // the word's value when block 0 of this tile's K range is NOT yet there
};
__device__ __forceinline__ int chase_ready(const Chase& ch, int v0, int v1) {
    const int a = v0 - ch.base0, b = v1 - ch.base1;
    return __builtin_amdgcn_readfirstlane(a < b ? a : b);
}
// leading K blocks of the tile that are complete: >= need on return, or the last value seen after a time-out (ok = false)
template <bool LOCALP = false>
__device__ __forceinline__ int chase_wait(const Chase& ch, int need, bool& ok) {
    int r = 0;
    if (!spin_until([&] { return (r = chase_ready(ch, poll_word(ch.p0), poll_word(ch.p1))) >= need; })) ok = false;
    acquire_unless_local<LOCALP>();
    return r;
}
// The two polls issued EARLY (their results are not waited for here): a tile puts them ahead of the loads of its input
// tile, so that one memory round trip covers both; chase_wait_pre then starts from what they brought.
struct ChasePre { int v0, v1; };
__device__ __forceinline__ ChasePre chase_issue(const Chase& ch) { return ChasePre{poll_word(ch.p0), poll_word(ch.p1)}; }
template <bool LOCALP = false>
__device__ __forceinline__ int chase_wait_pre(const Chase& ch, const ChasePre& pre, int need, bool& ok) {
    const int r = chase_ready(ch, pre.v0, pre.v1);
    if (r < need) return chase_wait<LOCALP>(ch, need, ok);
    acquire_unless_local<LOCALP>();
    return r;
}

// ---- waits of a workgroup -----------------------------------------------------------------------------------------------------
// thread 0 waits for one flag (4-cycle pause: the waiter is a tile in its pipeline) and acquires; the CALLER's next barrier
// covers the workgroup.  The result is meaningful in thread 0 only.
template <bool LOCALP = false>
__device__ __forceinline__ bool flag_wait_one_lane(const int* flag, int want = 0) {
    bool ok = true;
    if (threadIdx.x == 0) {
        ok = wait_word<IsSet, Pause4>(flag, want);
        acquire_unless_local<LOCALP>();
    }
    return ok;
}
// Thread 0 waits on up to two words, acquires once, reports a time-out; a barrier for the rest.  Two of them, because one
// template would put a test for nullptr on a word that one of its callers never leaves out:
//   batch_wait: the one-launch batched steps -- progress words (>=), either may be nullptr; Cmp0 = IsSet with want0 = 0: the
//               first word is a flag that carries a value (W_k's first word, a float's bits: tiles.h diag_body), up when non-zero
//   small_wait: the short-series step -- flags that equal the number of the step, a growing pause; f1 may be nullptr
template <bool LOCALP, class Cmp0 = AtLeast>
__device__ __forceinline__ void batch_wait(const int* p0, int want0, const int* p1, int want1, int* info_b) {
    if (threadIdx.x == 0) {
        bool ok = true;
        if (p0) ok = wait_word<Cmp0>(p0, want0);
        if (p1) ok = wait_word<AtLeast>(p1, want1) && ok;
        acquire_unless_local<LOCALP>();
        if (!ok) report_timeout(info_b);
    }
    __syncthreads();
}
__device__ __forceinline__ void small_wait(const int* f0, const int* f1, int want, int* info_b) {
    if (threadIdx.x == 0) {
        bool ok = wait_word<IsSet, PauseBackoff>(f0, want);
        if (f1) ok = wait_word<IsSet, PauseBackoff>(f1, want) && ok;
        acquire_unless_local<false>();
        if (!ok) report_timeout(info_b);
    }
    __syncthreads();
}

// ---- publishes (called by the whole workgroup) ---------------------------------------------------------------------------------
// behind plain stores: every storing wave drains, barrier, agent-scope release, the word.  LOCALP (readers on this XCD): the
// drain alone -- the stores are in this L2 -- and a plain store of the word, which keeps its line there for the polls.
// pub_tid: the thread that fences and stores the word -- a wave the caller's latency chain does not wait for, if it has one
template <bool LOCALP>
__device__ __forceinline__ void publish_release(int* word, int val, int pub_tid = 0) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if ((int)threadIdx.x == pub_tid) {
        if constexpr (LOCALP) {
            *reinterpret_cast<volatile int*>(word) = val;
        } else {
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // restate the wait the compiler may drop
            __hip_atomic_store(word, val, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}
// behind written-through (sc1) stores: every storing wave drains, barrier, the word -- nothing is left in L2 to write back
template <bool LOCALP>
__device__ __forceinline__ void publish_wt(int* word, int val) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) {
        if constexpr (LOCALP) *reinterpret_cast<volatile int*>(word) = val;
        else __hip_atomic_store(word, val, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// ---- who runs which piece: the puller queues of the one-launch batched steps ---------------------------------------------------
// Round 5 ran piece w as workgroup w and leaned on two things HIP does not promise (MI355X_MICROARCH.md, "Workgroup
// dispatch, XCD placement"): workgroups start in grid order (deadlock freedom) and workgroup w sits on XCD w % 8 (LOCAL's
// fence-free hand-offs through one L2).  Now the grid is a set of PULLERS -- as many workgroups as the chip holds at once,
// though nothing depends on that number -- and a piece is whatever the next ticket of a queue says:
//   * a waiter only ever waits for a piece with a SMALLER ticket of its own queue (the list is topologically ordered), and
//     a ticket is taken by a workgroup that is running: whatever is waited for is running or finished, whatever order
//     and wherever the dispatcher starts workgroups;
//   * LOCAL (batch a multiple of 8): eight queues, queue q = the pieces of the matrices b = q (mod 8) -- piece 8 t + q of
//     the list is ticket t of queue q, the list being matrix-innermost.  A workgroup asks the HARDWARE which XCD it is on
//     (s_getreg HW_REG_XCC_ID) and pulls from the queues that XCD owns; ownership is one compare-and-swap per queue
//     (claim[q] = XCD + 1): first its own number, and when that queue is dry, any queue nobody has claimed (an XCD that got
//     no workgroup at all -- a CU mask -- leaves an orphan that the others adopt whole).  So every piece of a matrix runs
//     under ONE L2 because the workgroups that run them read their own XCC_ID, not because of where workgroup w landed.
//   * otherwise: one queue, the agent-scope protocol, any workgroup anywhere.
// Queue words (ints, behind the progress words, cleared with them): head of queue q at [32 q], claim at [32 q + 1].
constexpr int BATCH_QWORDS = 8 * 32;

// HW_REG_XCC_ID (hwreg 20), bits 3:0: the XCD this wave runs on
__device__ __forceinline__ int hw_xcc_id() { return (int)__builtin_amdgcn_s_getreg((4 - 1) << 11 | 0 << 6 | 20) & 7; }

// Thread 0's view of the queues: which one it pulls from and how many it has tried to claim (see the block comment above).
//   xskew (tuning / tests): added to the hardware's XCC id -- the queues then sit on other XCDs than their numbers say;
//   xdrop (tuning / tests): bit x set = the workgroups on XCD x leave at once, as if a CU mask had emptied it -- their queues
//   are adopted by the others.
struct BatchPull {
    int q = -1, scan = 0;
};
template <bool LOCAL>
__device__ __forceinline__ int batch_next_piece(BatchPull& p, int* __restrict__ qw, int xcc, int per_queue) {
    for (;;) {
        if (p.q >= 0) {
            const int t = __hip_atomic_fetch_add(qw + 32 * p.q, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (t < per_queue) return LOCAL ? 8 * t + p.q : t;
            p.q = -1;
        }
        if (!LOCAL) {
            if (p.scan) return -1;
            p.scan = 1;
            p.q = 0;
            continue;
        }
        while (p.q < 0 && p.scan < 8) {
            const int cand = (xcc + p.scan) & 7;
            ++p.scan;
            int seen = __hip_atomic_load(qw + 32 * cand + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (seen == 0) {
                int expect = 0;
                if (__hip_atomic_compare_exchange_strong(qw + 32 * cand + 1, &expect, xcc + 1, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                                         __HIP_MEMORY_SCOPE_AGENT))
                    seen = xcc + 1;
                else
                    seen = expect;
            }
            if (seen == xcc + 1) p.q = cand;
        }
        if (p.q < 0) return -1;
    }
}

}  // namespace volt
