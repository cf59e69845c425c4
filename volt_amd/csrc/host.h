// Host-side internals shared by the translation units of libvolt_hip.so (not part of the C ABI): the tuning table, the
// argument bundles, and EVERY function that crosses a translation unit -- declared here once, defined in the file named
// beside it, declared nowhere else.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include <mutex>

// Schedule parameters: compiled-in defaults (measured on MI355X).  A deployment reads NO environment:
// only a process started with VOLT_TUNE=1 (the experiment scripts) may override them through the VOLT_* variables listed in
// include/volt_hip_tune.h -- read ONCE, by read_env in runtime.hip when tunables() is first called, nowhere else.
struct Tunables {
    int groups = 2;                  // stream groups of a large batch (2 >= 4 > 8 with one launch per block column)
    int splitk_target = 512, splitk_minl = 2, splitk_maxs = 8, splitk_groups = 2, splitk_maxb = 22;
    int sched = 1, sched_minb = 3, sched_maxb = 31, sched_maxb_potrf = 64;
    int sched_g = 256, sched_s = 4, sched_groups = 2, sched_kmin = -1;
    float sched_frac = 0.6f;
    int small_nmax = 8, small_maxwg = 1150;    // the one-launch step: block columns it takes, and workgroups at most
    int plain_spread = 320, split_spread = 700;   // plain / all-split launches of up to this many workgroups run one workgroup per CU
    int long_split = 1;                      // long series: the spine split in two workgroups (substitution | rank-32 updates + diagonal block)
    int long_xcd = 0;                        // long series: spines on one XCD, their hand-offs through its L2 (long_sched.h)
    int long_on = 1, long_first = 0, long_emin = 1, long_pad = 1, long_nmin = 2;   // one long series in one launch: on/off, last slice's blocks (0: 3 up to 24 block columns, 4 above), shortest sliced early part, a CU per workgroup, block columns above which it takes one series
    int small_maxb = 40, small_maxb2 = 64;     // ... series at most (three or four block columns / one or two)
    int small_pad_maxb = 40;                   // ... up to this many series with a CU per workgroup (16 KB of LDS padding)
    // ---- topology (round 5).  Every gate above was measured on a full MI355X: 256 CUs in 8 XCDs.  The device is asked once
    // (multiprocessor count, hipDeviceAttributeNumberOfXccs); on anything else -- a partitioned (CPX / DPX) or otherwise
    // reduced device -- the slot-count gates are scaled with the CU count and the one-launch steps, whose tuning AND whose
    // one-XCD-per-matrix hand-offs assume the full chip, are switched off: such a device runs the launch-per-column schedules.
    int cus = 256, xccs = 8;
    int group_gate = 700;                      // launches of fewer workgroups than this run as one stream group
    int batch = 1;                             // the whole batched step in one launch (batch_step.hip): 0 off, 1 where measured faster, 2 wherever it can run
    int batch_order = -1;                      // ... order of a block column's tiles in its list: -1 by shape (batch_step.hip, batch_order_for), 0 matrix innermost, 1 matrix-major, 2 + 4 log2(window) + 32 (groups side by side - 1) windowed (batch_sched.h)
    int batch_lad = 0;                         // ... its look-ahead tiles listed this many block columns early (batch_sched.h).  Measured, ms/step at lad 0 / 1 / 2 / 3: 8 x 4096 3.64 / 3.65 / 3.68 / 3.69, 16 x 4096 5.94 / 5.95 / 6.00 / 6.13, 64 x 4096 21.95 / 21.98 / 21.99 / 22.01: no gain, off
    int batch_spread = 400;                    // ... with up to this many tiles per block column, B (n + 1), it runs ONE workgroup per CU.  ms/step two per CU -> one per CU at N = 4096: B = 2 1.90 -> 1.66, 4 2.57 -> 2.10, 8 3.64 -> 3.37, 12 4.80 -> 4.82, 16 5.89 -> 6.16, 24 8.51 -> 9.17; at N = 2048: B = 8 0.99 -> 0.82, 16 1.28 -> 1.11.  Shorter series cross over later (their tiles are shorter, the chain weighs more): + 9 tiles per block column short of 32 -- 24 x 2048 (408 tiles) 1.59 -> 1.48, 32 x 2048 (544) 1.840 -> 1.836, 64 x 2048 (1088) 3.26 -> 3.52; 32 x 1536 (416) 1.02 -> 0.92; 64 x 1024 (576) 0.70 -> 0.67, 40 x 1024 0.58 -> 0.48; 16 x 3072 (400) 2.92 -> 2.87, 24 x 3072 (600) 3.97 -> 4.21
    int batch64 = 1;                           // the fp64 factorisation / gradient step in one launch (batch64_step.hip): 0 off, 1 where measured faster, 2 wherever it can run
    int batch64_max = 3300;                    // ... up to this many tiles per block column, B (n + 1) (one workgroup per CU: the diagonal block's 133 KB image).  Measured against chol64.hip's schedules (profiles/r05/batch64_gate_sweep.txt, _large.txt): the factorisation 1.06 - 2.17 x at every shape tried, 1 .. 512 matrices of N = 512 .. 4096 (up to 3264 tiles); the gradient step 1.01 - 1.90 x (96 x 4096, 3168 tiles: 1.01; 96 x 3072, 2400: 1.05): its limit from 24 block columns on is batch64_max_step
    int batch64_max_step = 2500;
    int batch_local = 1;                       // ... batches that are a multiple of 8 hand their tiles on through the XCD's L2 (0: the agent-scope protocol everywhere)
    int batch_pullers = 1;                     // ... its grid: this many times the workgroups the chip holds at once, pulling pieces by ticket (0: one workgroup per piece -- they pull all the same)
    int long_pullers = 1;                      // one long series: this many times the resident workgroups pull its pieces by ticket (0: a workgroup per piece -- they take tickets all the same)
    int rollout_lane = 1;                      // rollouts: one lane per path where the mean's window fits the LDS ring (0: a wave per path everywhere -- the tests compare the two)
    int batch_xskew = 0, batch_xdrop = 0;      // ... tests only: the queues of the XCDs shifted by this many (the map is nobody's assumption); bit x set = the pullers on XCD x leave at once (an XCD a CU mask emptied: its queue is adopted)
    // ---- chol64.hip's launch-per-column schedules.  The two slot counts are for the full chip: scaled with the CU count where they are used
    int f64_lookahead = -1;                    // columns of look-ahead: -1 by batch size (one below 6 matrices, two from 6 on), 0 one stream
    int f64_trtri_lookahead = -1;              // one-row look-ahead of the inverse: -1 up to 4 matrices, 0 off, 1 on
    int f64_spread = 512;                      // launches of up to this many workgroups run one workgroup per CU
    int f64_split_target = 512;                // K-sliced launches aim at this many workgroups
};
const Tunables& tunables();                    // runtime.hip: the table above after the environment (VOLT_TUNE=1 only) and the device's topology, made once per process

namespace volt {

inline size_t al256(size_t x) { return (x + 255) & ~(size_t)255; }   // every region of a workspace starts on a 256-byte boundary

// ---- what the tile bodies read their input from, and the reductions fused into the inverse (plain data: no device code)
// C tiles of block columns >= 1 come straight from the caller's K (+ sigma2/jitter on the diagonal, identity in the
// padding) instead of a prepared copy in A, which removes the K -> A copy pass for every block column but the first.
struct KSource {
    const float* K;          // nullptr: the working matrix A already holds the input (volt_potrf_f32)
    int64_t ldk, bsk;
    const float* sigma2;
    float jitter;
    int N;
};
// Where the fp64 one-launch step reads a tile of its input from (batch64_step.hip): K == nullptr -- the prepared copy A; else the
// caller's K (+ sigma2[b] + jitter on the diagonal, identity in the padding): no copy-in pass ahead of the factorisation.
struct KSource64 {
    const double* K;
    int64_t ldk, bsk;
    const double* sigma2;
    double jitter;
    int N;
};
// Optional reductions fused into the trtri epilogue (the MLL step needs z = Y'r and ||Y||_F^2; doing
// them here saves a full pass over Y): zpart[b][j][i*128 + r] = sum_c Y[j*128+c][i*128+r] rvec[j*128+c],
// frob[b][tile(j,i)] = sum of squares over rows < N.  Deterministic, no atomics.
struct TriReduce {
    const float* rpad;   // [B,Np] residual, zero padded; nullptr = no reductions
    float* zpart;        // [B,n,Np]
    float* frob;         // [B,n(n+1)/2]
    int N;
};

// ---- argument bundles of the functions below (host only; none of them is a kernel argument)
struct StepMats {            // the matrices of an fp32 step
    float *A, *Winv, *Y;     // Y == nullptr: the factorisation alone
    int* info;
    int B, N;                // N: the series' length (the padded size where A holds the input)
    hipStream_t stream;
};
struct StepMats64 {          // ... of an fp64 one (always padded)
    double *A, *Winv, *Y;
    int* info;
    int B, Np;
    hipStream_t stream;
};
struct StepTail {            // the vectors of a step's O(N^2) tail
    const float* resid;
    float *rpad, *z, *apad, *apart, *out, *alpha;
};
struct Region {              // a state region of the caller's workspace
    void* p = nullptr;
    size_t bytes = 0;
};
struct Carver {              // walks the caller's workspace region by region; base == nullptr: the sizes alone (off, at the end, is the total)
    void* base;
    size_t off = 0;
    template <typename T> T* take(size_t count) {
        T* p = base && count ? reinterpret_cast<T*>(static_cast<char*>(base) + off) : nullptr;
        off += al256(count * sizeof(T));
        return p;
    }
    Region region(size_t bytes) { return Region{take<char>(bytes), bytes}; }
    void skip(size_t bytes) { off += al256(bytes); }     // a workspace embedded at the front (the GPCV layouts begin with the MLL step's)
};
struct SplitScratch {        // scratch of the K-sliced / balanced launch-per-column schedules
    float* slab;
    int* count;
    int rows;
    Region tab;              // the balanced schedule's tables (p == nullptr: the workspace was not declared initialised)
};
struct ProfileOut {          // volt_profile_step_f32's host outputs
    float *ms_sum, *ms_union;
    int* launches;
    float* per_launch;
};

// "hand-offs through the XCD's L2": eight queues, one per XCD, when the matrices divide among them evenly (the pullers read their XCC id)
inline bool batch_local_handoffs(int B) { return (B & 7) == 0 && tunables().batch_local != 0 && tunables().xccs == 8; }
// grid of a begin kernel (256 threads): a thread of its own for each of the first `direct` words, at most 256 workgroups striding over the rest
inline int begin_grid(int direct, int strided) {
    int blocks = ((direct > strided ? direct : strided) + 255) / 256;
    if (blocks > 256) blocks = 256;
    if (blocks * 256 < direct) blocks = (direct + 255) / 256;
    return blocks;
}

}  // namespace volt

// ---- runtime.hip: the process-wide state -- tunables() above and the stream pool of the current device (nullptr: none).
// chol.hip's stream groups and chol64.hip's look-ahead schedules run on it, under its mutex while they enqueue
constexpr int MAX_GROUPS = 8;
struct StreamPool {
    hipStream_t aux[MAX_GROUPS - 1];
    hipEvent_t fork, join[MAX_GROUPS - 1], extra[5];     // extra: chol64.hip's look-ahead schedules
    std::mutex mu;
    int want_groups = 2;                 // tunables().groups
    bool ok = false;
};
StreamPool* stream_pool();
// ---- chol.hip: the launch-per-column schedules
// runs the factorisation group by group on the library's streams and calls `post` on each group's stream when that
// group's factor (+ inverse) is enqueued, so the O(N^2) tail of one group overlaps the other groups' MFMA work
typedef void (*volt_group_post_fn)(void* ctx, int b0, int Bg, hipStream_t s);
size_t volt_internal_sched_bytes(int B, int n);
int volt_internal_sched_install(volt::Region tab, int B, int n, int has_y, int cap, void* stream);
int volt_internal_factor(const volt::StepMats& m, const volt::KSource& src, const volt::TriReduce& red, const volt::SplitScratch& sk,
                         volt_group_post_fn post, void* post_ctx);
int volt_internal_profile(const volt::StepMats& m, const volt::KSource& src, const volt::TriReduce& red, const volt::SplitScratch& sk,
                          int groups, volt_group_post_fn post, void* post_ctx, const volt::ProfileOut& out);
// ---- one_launch.hip: short series / one long series in one launch.  A step returns 1: enqueued, 0: not this shape's, else a HIP error
size_t volt_internal_small_bytes(int B, int n);
int volt_internal_small_install(volt::Region state, int B, int n, void* stream);
int volt_internal_small_step(const volt::StepMats& m, const volt::KSource& src, const volt::TriReduce& red, const volt::StepTail& t,
                             volt::Region state);
size_t volt_internal_long_bytes(int B, int n);
size_t volt_internal_long_slab_floats(int B, int n);
int volt_internal_long_install(volt::Region state, int B, int n, void* stream);
int volt_internal_long_step(const volt::StepMats& m, const volt::KSource& src, const volt::TriReduce& red, const volt::StepTail& t,
                            float* eslab, volt::Region state);
// ---- batch_step.hip: the whole batched step in one launch (e0 / e1: events recorded around the step kernel)
bool volt_internal_batch_applies(int B, int n, int has_y);
size_t volt_internal_batch_bytes(int B, int n, int has_y);
bool volt_internal_batch_first();
int volt_internal_batch_install(volt::Region state, int B, int n, int has_y, void* stream);
int volt_internal_batch_step(const volt::StepMats& m, const volt::KSource& src, const volt::TriReduce& red, const volt::StepTail& t,
                             volt::Region state, hipEvent_t e0 = nullptr, hipEvent_t e1 = nullptr);
// ---- chol64.hip, batch64_step.hip: the fp64 factorisation (+ inverse) launch per column / in one launch (state: its progress words)
int volt_internal_factor_f64(const volt::StepMats64& m, volt::Region state = {});
bool volt_internal_batch64_applies(int B, int n, int has_y);
size_t volt_internal_batch64_bytes(int B, int n, int has_y);
int volt_internal_batch64_step(const volt::StepMats64& m, volt::Region state, const volt::KSource64* ksrc = nullptr);
size_t volt_internal_batch64_trtri_bytes(int B, int n);
int volt_internal_batch64_trtri(const double* A, const double* Winv, double* Y, int B, int Np, volt::Region state, void* stream);
// ---- mll.hip: gpcv.hip continues from the factor and Y = L^-T the step leaves in its workspace
const float* volt_internal_mll_y(void* workspace, int B, int N);
// ---- gpcv.hip: the variational step's likelihood rows ("exp": abc == nullptr, else "cv" + the fixed-order reduction into
// grad_abc; rowstat [B,N,4], cvpart [B, ceil(N/4), 3 Kc]) and its scalars (out [B,12] from rowstat, an MLL-style out [B,8] and
// per-series "tile" sums of tr(K^-1 S) and |G|_F^2), for gpcv_bm.hip
int volt_internal_gpcv_rows(const float* m, const float* Lq, const float* y, const float* abc, int Kc, const float* gh_x,
                            const float* gh_w, int Q, float min_var, float min_scale, float w_ell, float* rowstat, float* cvpart,
                            float* grad_abc, int B, int N, hipStream_t s);
int volt_internal_gpcv_scalars(const float* rowstat, const float* mllout, const float* frobT, const float* frobG, float jitter,
                               float* out, int B, int N, int ntiles, float w_ell, float w_kl, hipStream_t s);
// ---- bm.hip: its entries (volt_bm_*) are the C ABI's, declared and documented in include/volt_hip.h.  gpcv_bm.hip continues from
// the pivots' reciprocals 1/d_i that volt_bm_step_* (VOLT_WANT_GRAD) leaves in its workspace: fp64, [N][B] series-fastest
const double* volt_internal_bm_inv(const void* workspace);
