// resco_sim.hip -- MI355X (gfx950 / CDNA4) batched traffic-signal microsimulator behind the C ABI of
// include/resco_sim.h.  Written for gfx950 only: wave64, LDS-resident environment state, one workgroup
// per environment instance, every tick of an env-step fused into ONE kernel launch.
//
// Hot path replaced (RESCO, paths relative to its repository):
//   MultiSignal.step                 resco_benchmark/multi_signal.py:164-197
//   Signal.prep_phase / set_phase    resco_benchmark/traffic_signal.py:176-187
//   sumo.simulationStep() x 10       resco_benchmark/multi_signal.py:102-105   (SUMO itself: [SUMO-K])
//   Signal.observe / get_vehicles    resco_benchmark/traffic_signal.py:189-247
//   states.drq_norm / mplight / wave resco_benchmark/states.py:34-127
//   rewards.wait / wait_norm / pressure  resco_benchmark/rewards.py:6-41
//
// Layout
//   HBM  : env-major SoA, field[env][slot]; a workgroup streams its env's slab in once per env-step
//          (coalesced, slot-contiguous), keeps it in LDS for all ticks, and streams it out once.
//   LDS  : per-vehicle nodes / arrays + list heads per 64 m cell + approach registers + per-lane aggregates.
//   L2/IC: read-only scenario tables shared by all environments (< 1 MB).
// There is no dense contraction on this path: no MFMA.  Arithmetic is IEEE fp32 with contraction off so the
// CPU oracle (oracle/resco_oracle.c, test-only) reproduces every value bit-for-bit.
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <math.h>
#include <initializer_list>
#include <mutex>
#include <new>
#include <string>
#include <vector>

#include "resco_sim.h"

// ---- what resco_step.h asks of its includer (the GPU flavour: LDS atomics, one thread per call of a phase)
#define RS_DEV __device__ __forceinline__
#define RS_HD __host__ __device__
#define RS_MEM __device__ __forceinline__
#define RS_G(p) (p)
#define RS_CARVE __host__ __device__ __forceinline__
__device__ __forceinline__ void rs_atomic_min(int32_t *p, int32_t v) { atomicMin(p, v); }
__device__ __forceinline__ void rs_atomic_min(uint32_t *p, uint32_t v) { atomicMin(p, v); }
__device__ __forceinline__ void rs_atomic_max(int32_t *p, int32_t v) { atomicMax(p, v); }
__device__ __forceinline__ void rs_atomic_add(int32_t *p, int32_t v) { atomicAdd(p, v); }
__device__ __forceinline__ int32_t rs_atomic_fetch_add(int32_t *p, int32_t v) { return atomicAdd(p, v); }
// the lanes of a wave that are here together take consecutive tickets from ONE atomic (the counter is the same for all of them)
__device__ __forceinline__ int32_t rs_wave_ticket(int32_t *p) {
    const unsigned long long m = __ballot(1);
    const int below = (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
    int32_t base = 0;
    if (below == 0) base = atomicAdd(p, (int32_t)__popcll(m));
    return __builtin_amdgcn_readlane(base, __ffsll((long long)m) - 1) + below;
}
// one atomic per wave instead of one per lane (64 lanes adding to ONE LDS address are served one after the other): called
// where the whole wave is converged
__device__ __forceinline__ void rs_wave_add(int32_t *p, int32_t v) {
    for (int m = 32; m > 0; m >>= 1) v += __shfl_xor(v, m);
    if ((threadIdx.x & 63) == 0 && v) atomicAdd(p, v);
}
__device__ __forceinline__ void rs_wave_max(int32_t *p, int32_t v) {
    for (int m = 32; m > 0; m >>= 1) { const int32_t o = __shfl_xor(v, m); v = o > v ? o : v; }
    if ((threadIdx.x & 63) == 0) atomicMax(p, v);
}
__device__ __forceinline__ void rs_atomic_or(uint32_t *p, uint32_t v) { atomicOr(p, v); }
__device__ __forceinline__ uint32_t rs_atomic_fetch_or(uint32_t *p, uint32_t v) { return atomicOr(p, v); }
__device__ __forceinline__ int rs_atomic_inc(int32_t *p) { return atomicAdd(p, 1); }
__device__ __forceinline__ void rs_atomic_and(uint32_t *p, uint32_t v) { atomicAnd(p, v); }
__device__ __forceinline__ uint32_t rs_atomic_cas(uint32_t *p, uint32_t cmp, uint32_t v) { return atomicCAS(p, cmp, v); }
__device__ __forceinline__ int rs_ffsll(unsigned long long x) { return __ffsll(x); }
__device__ __forceinline__ int rs_clzll(unsigned long long x) { return __clzll((long long)x); }
__device__ __forceinline__ int rs_ffs(uint32_t x) { return __ffs((int)x); }
__device__ __forceinline__ int rs_popc(uint32_t x) { return __popc(x); }
__device__ __forceinline__ float rs_int_as_float(int x) { return __int_as_float(x); }
__device__ __forceinline__ int rs_float_as_int(float x) { return __float_as_int(x); }
__device__ __forceinline__ uint16_t rs_f2h(float x) { return __half_as_ushort(__float2half(x)); }

// a / b by the hardware's Newton sequence without the range scaling (resco_step.h: RS_DIV).  Identical to `/` -- the same v_rcp_f32 and the same
// seven operations -- for finite non-zero b, a = 0 or 2^-100 < |a|, |a / b| and |1 / b| normal: every division of the step kernel
#ifndef RS_IEEE_DIV
__device__ __forceinline__ float rs_div_unscaled(float a, float b) {
    const float r0 = __builtin_amdgcn_rcpf(b);
    const float r1 = __builtin_fmaf(__builtin_fmaf(-b, r0, 1.0f), r0, r0);
    const float q0 = a * r1;
    const float q1 = __builtin_fmaf(__builtin_fmaf(-b, q0, a), r1, q0);
    return __builtin_fmaf(__builtin_fmaf(-b, q1, a), r1, q1);
}
#define RS_DIV(a, b) rs_div_unscaled((a), (b))
#endif
// all four dwords of a Node are "used": the compiler reads them with one ds_read_b128 instead of narrowing the read to the fields a loop
// body happens to need (resco_step.h: node_load)
#define RS_OPAQUE_S(x) asm volatile("" : "+s"(x));
#ifndef RS_NARROW_NODE
#define RS_KEEP4(a, b, c, d) asm volatile("" : "+v"(a), "+v"(b), "+v"(c), "+v"(d));
#endif
extern __shared__ __attribute__((aligned(16))) char rs_smem[];      // THE working memory of a workgroup (dynamic LDS)
#define RS_SMEM rs_smem

#ifdef RS_STUDY_SECTIONS       // study build: where inside the long path of the plan a wave's time goes (tools/phase_profile.py --sections)
__device__ unsigned long long *g_sec_prof;
#define RS_SEC_BEGIN unsigned long long sec_t = wall_clock64();
#define RS_SEC(id) { const unsigned long long sec_1 = wall_clock64(); if (g_sec_prof && (threadIdx.x & 63) == 0 && (blockIdx.x & 15) == 0) atomicAdd(&g_sec_prof[id], (sec_1 - sec_t) + (1ull << 40)); sec_t = wall_clock64(); }
#endif
#ifdef RS_DEVICE_ASSERT        // the CHECKING build (resco_amd/build.py: libresco_sim_check.so): the classification invariants of the step kernel -- a vehicle
// without FL_H never needs the walk over the links, one without FL_MH never leaves its lane -- are counted per environment in
// rs_stats()[11] instead of compiled out; tests/test_gpu_parity.py::test_device_invariant_counter holds the count at zero.  They rest
// on classify() and the plan evaluating the same floating-point expressions to the same bits at different inline sites
// (-ffp-contract=off): the one place where a compiler upgrade could silently skip a stop line.
#define RS_ASSERT(c) if (!(c)) rs_atomic_add(&L.sc[SC_STATS + ST_INVARIANT], 1);     // (`L`: the working memory, in scope at every site)
#endif
#include "resco_host.h"
#include "resco_policy.h"
#include "resco_frap.h"
#include "resco_ppo.h"
#include "resco_ppo_train.h"
#include "resco_dqn_train.h"
#include "resco_frap_train.h"

// ------------------------------------------------------------------------------------------------ kernels
// The tables / state / output descriptors live in ONE constant block in device memory (StepArgs): passed by value they
// would pin ~70 SGPRs for the whole kernel (beyond ~100 the compiler spills SGPRs into VGPR lanes around every use);
// behind a const __restrict__ pointer every field is a re-loadable scalar load.
struct StepArgs { KTab T; State G; Out O; Lds L; };
// the block is read through the CONSTANT address space: scalar loads, and the compiler takes pointers loaded from it for
// global ones (global_load instead of flat_load, which would also tie up the LDS wait counter)
typedef const __attribute__((address_space(4))) StepArgs *StepArgsPtr;

// grid = n_envs workgroups (one environment each); blockDim.x = 64 * waves (<= 1024), normally one thread per slot.
// PROF: the build with the in-kernel timers (rs_phase_profile); the production kernels carry none of that code
template <bool PROF> struct DevExec {
    int B;
    int wave;                       // threadIdx.x / 64, wave-uniform: lives in a scalar register
    unsigned long long *prof;       // optional per-phase timers (rs_phase_profile)
    unsigned long long t0;
    template <class F> __device__ __forceinline__ void phase(int id, F f) {
        // The thread index is RECOMPUTED per phase from the wave's index (a scalar) and the lane's position in the wave (two VALU
        // instructions): kept in a register across the kernel it costs a VGPR the 64-VGPR build does not have (it lived in scratch
        // and was re-loaded at the top of every phase), and an index the compiler can see through has every address derived from
        // it (the small strided loops of the tick's phases) computed once before the tick loop and kept alive across it --
        // 18 VGPRs spilled to scratch (round 2).
        int w = wave;
        uint32_t ones = ~0u;
        asm volatile("" : "+s"(w), "+s"(ones));     // (opaque: neither the lane index nor anything derived from it is hoisted out of the phase)
        int tid = (w << 6) | (int)__builtin_amdgcn_mbcnt_hi(ones, __builtin_amdgcn_mbcnt_lo(ones, 0u));
        asm volatile("" : "+v"(tid));
        f(tid);
        __syncthreads();
        if (PROF && prof) {         // (t0 stays wave-uniform: every thread takes the time, thread 0 adds it up)
            const unsigned long long t1 = wall_clock64();
            if (tid == 0) atomicAdd(&prof[id], t1 - t0);
            t0 = t1;
        }
    }
    // tid / 64 as a wave-uniform value: what is derived from it (the roles of the waves inside a phase) stays in scalar registers
    __device__ __forceinline__ int wave_of(int) const { return wave; }
    // the next work chunk of this wave: one LDS atomic per wave (called with the wave converged), broadcast from its first lane
    __device__ __forceinline__ int next_chunk(int32_t *ctr, int, int, int) const {
        int c = 0;
        if (__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)) == 0) c = atomicAdd(ctr, 1);
        return __builtin_amdgcn_readfirstlane(c);
    }
    // time a wave spends in one role of a phase: sum of the 100 MHz ticks in the low 40 bits, number of waves above
    __device__ __forceinline__ unsigned long long role_begin() const { return (PROF && prof) ? wall_clock64() : 0ull; }
    __device__ __forceinline__ void role_end(int id, unsigned long long start) const {
#ifdef RS_STUDY_SECTIONS
        return;
#endif
        if (PROF && prof && (threadIdx.x & 63) == 0 && (blockIdx.x & 15) == 0) atomicAdd(&prof[id], (wall_clock64() - start) + (1ull << 40));   // (every 16th environment: the sum stays below 2^40)
    }
};
// Register budgets: 64 VGPRs (eight waves per SIMD: FOUR 512-thread workgroups per CU -- the default where the working memory of an
// environment fits four times, round 6) and 80 VGPRs (three 512-thread workgroups per CU; `_v128` is the same code under a third
// launch bound); CAP = the slot capacity as a compile-time constant (0: any).
template <int CAP, bool PROF> __device__ __forceinline__ void rs_step_kernel_body(StepArgsPtr Ac, const KParams &P, const int32_t *__restrict__ actions) {
    if ((int)blockIdx.x >= P.n_envs) return;
    const StepArgs *A = (const StepArgs *)Ac;
#ifdef RS_STUDY_SECTIONS
    if (threadIdx.x == 0) g_sec_prof = P.prof;
#endif
    DevExec<PROF> ex{(int)blockDim.x, __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6), PROF ? P.prof : nullptr, (PROF && P.prof) ? wall_clock64() : 0ull};
    rs_step_body<CAP>(ex, A->L, A->T, A->G, A->O, P, actions, (int)blockIdx.x);
}
template <int CAP>
__global__ void __launch_bounds__(1024, 8)
rs_step_kernel_v64(StepArgsPtr Ac, KParams P, const int32_t *__restrict__ actions) { rs_step_kernel_body<CAP, false>(Ac, P, actions); }
template <int CAP>
__global__ void __launch_bounds__(768, 6)
rs_step_kernel_v80(StepArgsPtr Ac, KParams P, const int32_t *__restrict__ actions) { rs_step_kernel_body<CAP, false>(Ac, P, actions); }
template <int CAP>
__global__ void __launch_bounds__(512, 4)
rs_step_kernel_v128(StepArgsPtr Ac, KParams P, const int32_t *__restrict__ actions) { rs_step_kernel_body<CAP, false>(Ac, P, actions); }
// the profiling build (rs_phase_profile / RS_STUDY_SECTIONS): any capacity, 80 VGPRs
__global__ void __launch_bounds__(768, 6)
rs_step_kernel_prof(StepArgsPtr Ac, KParams P, const int32_t *__restrict__ actions) { rs_step_kernel_body<0, true>(Ac, P, actions); }

// reset / fresh Signal objects / the static agents: the bodies are in resco_host.h (shared with the host emulation)
__global__ void rs_reset_kernel(KTab T, State G, KParams P) { rs_reset_env(T, G, P, (int)blockIdx.x, (int)threadIdx.x, blockDim.x); }
__global__ void rs_reinit_kernel(KTab T, State G, KParams P) { rs_reinit_env(T, G, P, (int)blockIdx.x, (int)threadIdx.x, blockDim.x); }
__global__ void rs_act_random_kernel(KTab T, KParams P, uint32_t step_key, int32_t *actions) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < P.n_envs * T.n_signals) actions[i] = rs_random_action(T, P, step_key, i);
}
__global__ void rs_act_maxwave_kernel(KTab T, KParams P, const int32_t *pairs, int n_pairs, const int32_t *valid, const int32_t *order,
                                      int use_pressure, const int32_t *mplight, const int32_t *wave, int32_t *actions) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < P.n_envs * T.n_signals) actions[i] = rs_maxwave_action(T, pairs, n_pairs, valid, order, use_pressure, mplight, wave, i);
}

// ------------------------------------------------------------------------------------------------ host side
enum RegBudget { V64 = 0, V128 = 1, V80 = 2 };      // VGPRs of the step kernel a handle launches (the index step_kernel_for takes)
struct rs_sim {
    int device = 0;
    int n_envs = 0, env_base = 0, block = 256;
    int ratio = 1;                  // rs_params.step_ratio: simulation ticks per step_sim() call
    size_t lds = 0;
    KTab K{};
    StepArgs *args = nullptr;      // device copy of {K, G, O}
    RegBudget budget = V64;
    State G{};
    Out O{};
    KParams P{};
    uint32_t out_mask = OUT_ALL;        // rs_set_outputs
    int32_t *actions = nullptr;
    int32_t *pairs = nullptr, *valid = nullptr, *order = nullptr;
    unsigned long long *prof = nullptr;
    int n_pairs = 0;
    hipStream_t stream = nullptr;
    hipStream_t last = nullptr;         // stream of the most recent launch: what the synchronous calls wait for
    std::vector<void *> allocs;
    Buf bufs[RS_BUF_COUNT]{};
    bool timing = false;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> events;
    size_t ev_used = 0;
    std::string err;
};

static thread_local std::string g_create_err;

#define HIPCHK(h, call)                                                                            \
    do {                                                                                           \
        hipError_t e_ = (call);                                                                    \
        if (e_ != hipSuccess) {                                                                    \
            (h)->err = std::string(#call) + ": " + hipGetErrorString(e_);                          \
            (void)hipGetLastError();    /* the error is reported here: do not leave it for the next hipGetLastError() */ \
            return RS_EHIP;                                                                        \
        }                                                                                          \
    } while (0)

template <typename Tp>
static int dev_alloc(rs_sim *h, Tp **p, size_t count, bool zero = true) {
    void *d = nullptr;
    size_t bytes = (count ? count : 1) * sizeof(Tp);
    hipError_t e = hipMalloc(&d, bytes);
    if (e != hipSuccess) { h->err = std::string("hipMalloc: ") + hipGetErrorString(e); return RS_ENOMEM; }
    if (zero) (void)hipMemset(d, 0, bytes);
    h->allocs.push_back(d);
    *p = (Tp *)d;
    return RS_OK;
}
template <typename Tp>
static int dev_upload(rs_sim *h, const Tp **dst, const Tp *src, size_t count) {
    Tp *d = nullptr;
    int rc = dev_alloc(h, &d, count, false);
    if (rc) return rc;
    if (count) HIPCHK(h, hipMemcpy(d, src, count * sizeof(Tp), hipMemcpyHostToDevice));
    *dst = d;
    return RS_OK;
}

typedef void (*step_kernel_fn)(StepArgsPtr, KParams, const int32_t *);
static const int kStepCaps[] = {0, 128, 256, 512, 768, 896, 1024};
// regs (a RegBudget): 64 VGPRs (blocks up to 1024 threads), 128 VGPRs (up to 512), 80 VGPRs (up to 768)
#define RS_PICK(cap_) (regs == V128 ? rs_step_kernel_v128<cap_> : (regs == V80 ? rs_step_kernel_v80<cap_> : rs_step_kernel_v64<cap_>))
static step_kernel_fn step_kernel_for(int regs, int capacity) {
#ifdef RS_ONE_CAP       // study builds (seconds instead of minutes to compile): one capacity, the 64- and the 80-VGPR kernel only
    (void)capacity;
    return regs == V64 ? rs_step_kernel_v64<RS_ONE_CAP> : rs_step_kernel_v80<RS_ONE_CAP>;
#else
    switch (capacity) {
        case 128: return RS_PICK(128);
        case 256: return RS_PICK(256);
        case 512: return RS_PICK(512);
        case 768: return RS_PICK(768);
        case 896: return RS_PICK(896);
        case 1024: return RS_PICK(1024);
        default: return RS_PICK(0);
    }
#endif
}

// every synchronous entry point waits for the handle's own stream AND the caller stream of the last launch
static hipError_t wait_idle(rs_sim *h) {
    hipError_t e = hipStreamSynchronize(h->stream);
    if (e == hipSuccess && h->last && h->last != h->stream) e = hipStreamSynchronize(h->last);
    return e;
}

// The workgroup shape rs_create picks for block_threads = 0 (include/resco_sim.h).  Base: one thread per TWO slots (the capacity is the
// episode's peak, about twice the typical occupancy), at most 512 threads, 80 VGPRs -- at large batches the fewest waves per
// environment win (cologne1, 128 slots: 64 threads 13.3 M env-steps/s against 12.5 M with 128 at 16 384 environments).  A SMALL batch
// leaves the chip empty at that shape -- 1024 environments x one wave are 4 waves per CU -- and a phase of the tick is the latency of
// its chunks one after the other on that wave: as long as the resident-wave budget of the device (7 waves per SIMD with the 80-VGPR
// build) holds every environment at once, the environment gets more waves, up to one per chunk of a phase (capacity / 64 slots chunks
// + one list chunk).  Measured on one MI355X, random policy (profiles/r06_block_sweep.txt): cologne1 x 1024 2.65 -> 4.94 M with 256
// threads, cologne8 x 2048 6.04 -> 6.88 M with 192, and at >= 4096 environments the base shape again.
extern "C" int32_t rs_default_block(int32_t capacity, int32_t n_envs_on_device, int32_t device_id) {
    const int C = capacity;
    if (C < 64 || n_envs_on_device <= 0) return 0;
    const int base = C >= 768 ? 8 : ((C / 2) + 63) / 64;            // waves
    int waves = base;
    if (C < 768) {          // (the large scenarios run three or four 512-thread workgroups per CU: more threads would lose one)
        int cus = 256;
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, device_id) == hipSuccess && prop.multiProcessorCount > 0) cus = prop.multiProcessorCount;
        else (void)hipGetLastError();
        const long budget = (long)cus * 4 * 7;                      // resident waves of the 80-VGPR build (what these shapes run with)
        const int fit = (int)(budget / n_envs_on_device), most = C / 64 + 1;
        waves = fit < most ? fit : most;
        if (waves < base) waves = base;
    }
    return -(20000 + 64 * waves);
}

// The block_threads argument of rs_create (include/resco_sim.h) as a register budget and a thread count; false: not a valid shape.
// A positive value is that many threads (at most 1024) of the 64-VGPR build; a negative value selects the 128-VGPR build with |value|
// threads (<= 512), -(10000 + threads) the 80-VGPR build (<= 768) -- tuning knobs; -(20000 + threads) is what
// rs_default_block proposes.
static bool decode_block(int block_threads, size_t lds, RegBudget *budget, int *threads) {
    int t = block_threads;
    RegBudget b = V64;
    if (t <= -20000) {
        // the shape rs_default_block proposes: the register budget follows from what fits a CU.  Where the working memory lets FOUR
        // 512-thread workgroups share a CU they need eight waves per SIMD, i.e. the 64-VGPR build (ingolstadt21 with 896 slots:
        // 40 768 B; +14 % env-steps/s over three workgroups of the 80-VGPR build, profiles/r06_ab_occupancy.txt); else 80 VGPRs
        t = -t - 20000;
        b = (t == 512 && lds <= RS_LDS_4WG_LIMIT) ? V64 : V80;
    } else if (t < 0) { b = V128; t = -t; if (t >= 10000) { b = V80; t -= 10000; } }
    *budget = b; *threads = t;
    return t % 64 == 0 && t >= 64 && t <= (b == V128 ? 512 : (b == V80 ? 768 : 1024));
}

extern "C" int rs_create(const rs_scenario *sc, const rs_params *p, int32_t n_envs, int32_t env_base, int32_t device_id,
                         int32_t block_threads, rs_handle *out) {
    if (!sc || !p || !out || n_envs <= 0) { g_create_err = "rs_create: bad argument"; return RS_EINVAL; }
    rs_sim *h = new (std::nothrow) rs_sim();
    if (!h) return RS_ENOMEM;
    auto fail = [&](int rc) { g_create_err = h->err; (void)hipGetLastError(); rs_destroy(h); return rc; };
    (void)hipGetLastError();        // a stale error of this thread (another library's, an earlier failed call) is not ours
    h->device = device_id; h->n_envs = n_envs; h->env_base = env_base;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { h->err = "no HIP device visible (this library has no CPU fallback)"; return fail(RS_EHIP); }
    if (hipSetDevice(device_id) != hipSuccess) { h->err = "hipSetDevice failed"; return fail(RS_EHIP); }
    if (sc->step_length <= 0 || sc->yellow_length < 0 || sc->yellow_length >= sc->step_length) {
        h->err = "need 0 <= yellow_length < step_length"; return fail(RS_EINVAL);
    }
    const int C = sc->capacity;
    if (C < 64 || (C % 64) || C > 1984) { h->err = "capacity must be a multiple of 64 in [64, 1984]"; return fail(RS_ELIMIT); }
    if (sc->kmax < 1 || sc->kmax > 16) { h->err = "kmax (lanes per edge) must be in [1, 16]"; return fail(RS_ELIMIT); }
    PackedTables PT;
    if (const char *msg = rs_pack_tables(PT, sc)) { h->err = msg; return fail(RS_ELIMIT); }
    int rc;
#define UP(dst, type, src, count) if ((rc = dev_upload<type>(h, &dst, src, (size_t)(count)))) return fail(rc);
    RS_KTAB_TABLES(UP, h->K, PT, sc)
#undef UP
    h->ratio = rs_step_ratio(p);
    rs_ktab_scalars(h->K, PT, sc, h->ratio);
    const int lmax = PT.lmax;
    h->P = rs_kparams(p, env_base, n_envs);
    const size_t N = (size_t)n_envs, NC = N * C, S = (size_t)sc->n_signals;
    State &G = h->G;
    Out &O = h->O;
    {
        char *slab = nullptr, *outb = nullptr;
        G.nc = NC;
        O.n = n_envs; O.o = sc->n_obs; O.s = sc->n_signals; O.lm = lmax;
        if ((rc = dev_alloc(h, &slab, State::bytes(NC))) || (rc = dev_alloc(h, &outb, O.bytes())) ||
            (rc = dev_alloc(h, &G.env, N * 4)) || (rc = dev_alloc(h, &G.tls, N * S * TLS_W)) || (rc = dev_alloc(h, &G.stats, N * ST_N)) ||
            (rc = dev_alloc(h, &G.dep_next, N * (size_t)h->K.n_dep)) || (rc = dev_alloc(h, &G.mail, N * (size_t)((C + 31) / 32))) ||
            (rc = dev_alloc(h, &h->actions, N * S)))
            return fail(rc);
        G.base = slab; O.base = outb;
    }
    G.trip_log = nullptr;
    if (p->trip_log && (rc = dev_alloc(h, &G.trip_log, N * (size_t)sc->n_trips * 4))) return fail(rc);
    rs_fill_bufs(h->bufs, G, O, h->actions, BufDims{n_envs, C, sc->n_signals, sc->n_obs, lmax, h->K.n_dep, p->trip_log ? sc->n_trips : 0});

    h->lds = lds_carve(nullptr, C, h->K.n_cells, h->K.n_arr, h->K.n_dep, sc->n_obs, sc->n_signals, sc->n_vtypes, h->K.tls_maxl);
    if (const char *pad = getenv("RESCO_STUDY_LDS_PAD")) h->lds += (size_t)atoi(pad);      // study knob: unused bytes, to hold the residency fixed in an A/B
    if (h->lds > 160 * 1024) { h->err = "scenario needs more than 160 KiB of LDS per environment"; return fail(RS_ELIMIT); }
    if (block_threads == 0) block_threads = rs_default_block(C, n_envs, device_id);
    if (!decode_block(block_threads, h->lds, &h->budget, &block_threads)) {
        h->err = "block_threads must be a multiple of 64 in [64, 1024] ([64, 768] for the 80-VGPR build, [64, 512] for the 128-VGPR build)";
        return fail(RS_EINVAL);
    }
    h->block = block_threads;
    {
        // the dynamic-LDS ceiling is an attribute of the kernel (per device), not of a launch: only ever raise it,
        // or a handle created earlier for a larger scenario could no longer launch
        static std::mutex mu;
        static size_t max_lds[64] = {0};
        std::lock_guard<std::mutex> lock(mu);
        size_t &cur = max_lds[device_id & 63];
        if (h->lds > cur) {
            for (int v = V64; v <= V80; ++v)
                for (int cp : kStepCaps)        // every instantiation: the ceiling is per kernel function
                    if (hipFuncSetAttribute((const void *)step_kernel_for(v, cp), hipFuncAttributeMaxDynamicSharedMemorySize, (int)h->lds) != hipSuccess) {
                        h->err = "hipFuncSetAttribute(MaxDynamicSharedMemorySize) failed"; return fail(RS_EHIP);
                    }
            if (hipFuncSetAttribute((const void *)rs_step_kernel_prof, hipFuncAttributeMaxDynamicSharedMemorySize, (int)h->lds) != hipSuccess) {
                h->err = "hipFuncSetAttribute(MaxDynamicSharedMemorySize) failed"; return fail(RS_EHIP);
            }
            cur = h->lds;
        }
    }
    {
        StepArgs sa{h->K, h->G, h->O, Lds{}};
        lds_carve(&sa.L, C, h->K.n_cells, h->K.n_arr, h->K.n_dep, sc->n_obs, sc->n_signals, sc->n_vtypes, h->K.tls_maxl);
        if (!lds_fix_matches(sa.L, C)) { h->err = "the layout of the working memory does not match the kernel's literals (lds_carve / LdsFix)"; return fail(RS_EINVAL); }
        sa.L.cell_inv = PT.cell_inv;
        if ((rc = dev_alloc(h, &h->args, 1, false))) return fail(rc);
        if (hipMemcpy(h->args, &sa, sizeof(sa), hipMemcpyHostToDevice) != hipSuccess) { h->err = "hipMemcpy(StepArgs) failed"; return fail(RS_EHIP); }
    }
    {   // The handle's stream gets a hardware queue of its OWN.  HIP multiplexes plain streams over GPU_MAX_HW_QUEUES (4) hardware
        // queues, least-used first, and two streams that share one run their kernels one after the other: pipes (several handles
        // per GPU whose launches are meant to overlap) lost a third of their rate whenever two of them met on a queue
        // (profiles/r05_pipes_group.txt).  A stream created with a CU mask is never multiplexed; the mask enables every CU.
        hipDeviceProp_t prop;
        std::vector<uint32_t> mask;
        if (getenv("RESCO_PLAIN_STREAMS") == nullptr && hipGetDeviceProperties(&prop, device_id) == hipSuccess)
            mask.assign((size_t)(prop.multiProcessorCount + 31) / 32, 0xFFFFFFFFu);
        if (mask.empty() || hipExtStreamCreateWithCUMask(&h->stream, (uint32_t)mask.size(), mask.data()) != hipSuccess) {
            (void)hipGetLastError();
            if (hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) != hipSuccess) { h->err = "hipStreamCreate failed"; return fail(RS_EHIP); }
        }
    }
    *out = h;
    int r2 = rs_reset(h, nullptr);
    if (r2) { g_create_err = h->err; *out = nullptr; rs_destroy(h); return r2; }
    return RS_OK;
}

extern "C" void rs_destroy(rs_handle h) {
    if (!h) return;
    (void)hipSetDevice(h->device);
    if (h->stream) { (void)wait_idle(h); (void)hipStreamDestroy(h->stream); }
    for (auto &e : h->events) { (void)hipEventDestroy(e.first); (void)hipEventDestroy(e.second); }
    for (void *p : h->allocs) (void)hipFree(p);
    delete h;
}

extern "C" const char *rs_last_error(rs_handle h) { return h ? h->err.c_str() : g_create_err.c_str(); }

static int launch_step(rs_sim *h, hipStream_t st, int n_ticks, int do_fsm, int do_observe = 1) {
    KParams P = h->P;
    P.n_ticks = n_ticks; P.do_fsm = do_fsm; P.do_observe = do_observe; P.out_mask = h->out_mask; P.prof = h->prof;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    if (h->timing) {
        if (h->ev_used == h->events.size()) {
            hipEvent_t a, b;
            HIPCHK(h, hipEventCreate(&a));
            HIPCHK(h, hipEventCreate(&b));
            h->events.emplace_back(a, b);
        }
        e0 = h->events[h->ev_used].first; e1 = h->events[h->ev_used].second;
        h->ev_used += 1;
        HIPCHK(h, hipEventRecord(e0, st));
    }
    // (the in-kernel timers live in a kernel of their own: any capacity, 80 VGPRs, at most 768 threads)
    const step_kernel_fn fn = (h->prof && h->block <= 768) ? (step_kernel_fn)rs_step_kernel_prof : step_kernel_for(h->budget, h->K.capacity);
    hipLaunchKernelGGL(fn, dim3(h->n_envs), dim3(h->block), h->lds, st, (StepArgsPtr)h->args, P, (const int32_t *)h->actions);
    HIPCHK(h, hipGetLastError());
    if (h->timing) HIPCHK(h, hipEventRecord(e1, st));
    return RS_OK;
}

// what every launching entry point begins with: the handle's device, and the stream of this launch (the caller's, or the handle's own)
static int enter(rs_sim *h, void *stream, hipStream_t *st) {
    if (!h) return RS_EINVAL;
    HIPCHK(h, hipSetDevice(h->device));
    *st = stream ? (hipStream_t)stream : h->stream;
    h->last = *st;
    return RS_OK;
}

// rs_reset / rs_reinit_signals: the kernel over the environments, then an untimed observe (of the new Signal objects)
static int launch_reset(rs_sim *h, void *stream, void (*kernel)(KTab, State, KParams)) {
    hipStream_t st;
    int rc = enter(h, stream, &st);
    if (rc) return rc;
    hipLaunchKernelGGL(kernel, dim3(h->n_envs), dim3(256), 0, st, h->K, h->G, h->P);
    HIPCHK(h, hipGetLastError());
    bool tm = h->timing;
    h->timing = false;
    rc = launch_step(h, st, 0, 0);
    h->timing = tm;
    return rc;
}
extern "C" int rs_reset(rs_handle h, void *stream) { return launch_reset(h, stream, rs_reset_kernel); }
extern "C" int rs_reinit_signals(rs_handle h, void *stream) { return launch_reset(h, stream, rs_reinit_kernel); }

extern "C" int rs_step(rs_handle h, const int32_t *actions, int32_t actions_on_device, void *stream) {
    hipStream_t st;
    if (int rc = enter(h, stream, &st)) return rc;
    if (actions) {
        size_t bytes = (size_t)h->n_envs * h->K.n_signals * sizeof(int32_t);
        HIPCHK(h, hipMemcpyAsync(h->actions, actions, bytes, actions_on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st));
        // a pageable host source may be read after the call returns: make the caller's buffer reusable
        if (!actions_on_device) HIPCHK(h, hipStreamSynchronize(st));
    }
    return launch_step(h, st, h->K.step_length * h->ratio, 1);
}

extern "C" int rs_ticks(rs_handle h, int32_t n_ticks, void *stream) {
    hipStream_t st;
    if (n_ticks < 0) return RS_EINVAL;
    if (int rc = enter(h, stream, &st)) return rc;
    return launch_step(h, st, n_ticks, 0);
}

extern "C" int rs_step_sim(rs_handle h, int32_t n_ticks, void *stream) {
    hipStream_t st;
    if (n_ticks < 0) return RS_EINVAL;
    if (int rc = enter(h, stream, &st)) return rc;
    return launch_step(h, st, n_ticks, 0, 0);
}

// which output buffers the observe of the following launches writes (bit b = buffer id b); the others keep their contents
extern "C" int rs_set_outputs(rs_handle h, uint64_t buffer_mask) {
    if (!h) return RS_EINVAL;
    h->out_mask = rs_out_mask(buffer_mask);
    return RS_OK;
}

extern "C" int rs_sync(rs_handle h) {
    if (!h) return RS_EINVAL;
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, wait_idle(h));
    return RS_OK;
}

// ---- the agents' launches: one function each, for the single call and for rs_group_step (the caller checks hipGetLastError)
static void launch_random(rs_sim *h, hipStream_t st, uint32_t step_key) {
    const int total = h->n_envs * h->K.n_signals;
    hipLaunchKernelGGL(rs_act_random_kernel, dim3((total + 255) / 256), dim3(256), 0, st, h->K, h->P, step_key, h->actions);
}
static void launch_maxwave(rs_sim *h, hipStream_t st, int use_pressure) {
    const int total = h->n_envs * h->K.n_signals;
    hipLaunchKernelGGL(rs_act_maxwave_kernel, dim3((total + 255) / 256), dim3(256), 0, st, h->K, h->P, (const int32_t *)h->pairs,
                       h->n_pairs, (const int32_t *)h->valid, (const int32_t *)h->order, use_pressure, (const int32_t *)h->O.mplight(),
                       (const int32_t *)h->O.wave(), h->actions);
}

extern "C" int rs_act_random(rs_handle h, uint32_t step_key, void *stream) {
    hipStream_t st;
    if (int rc = enter(h, stream, &st)) return rc;
    launch_random(h, st, step_key);
    HIPCHK(h, hipGetLastError());
    return RS_OK;
}

extern "C" int rs_act_maxwave(rs_handle h, const int32_t *phase_pairs, int32_t n_pairs, const int32_t *valid,
                              const int32_t *order, int32_t use_pressure, void *stream) {
    if (!h || n_pairs <= 0) return RS_EINVAL;
    // the agent reads the states.mplight / states.wave rows of the last observe: refuse when rs_set_outputs switched them off
    // (the buffer would hold stale rows, or zeros if it was never written)
    if (!(h->out_mask & (use_pressure ? OUT_MPLIGHT : OUT_WAVE))) {
        h->err = use_pressure ? "rs_act_maxwave(use_pressure=1) reads RS_BUF_MPLIGHT, which rs_set_outputs has switched off"
                              : "rs_act_maxwave(use_pressure=0) reads RS_BUF_WAVE, which rs_set_outputs has switched off";
        return RS_EINVAL;
    }
    hipStream_t st;
    if (int rc = enter(h, stream, &st)) return rc;
    if (!h->pairs) {
        if (!phase_pairs || !valid || !order) { h->err = "rs_act_maxwave: tables required on first use"; return RS_EINVAL; }
        int rc;
        if ((rc = dev_alloc(h, &h->pairs, (size_t)n_pairs * 2, false)) || (rc = dev_alloc(h, &h->valid, (size_t)h->K.n_signals * n_pairs, false)) ||
            (rc = dev_alloc(h, &h->order, (size_t)h->K.n_signals * n_pairs, false))) return rc;
        HIPCHK(h, hipMemcpy(h->order, order, (size_t)h->K.n_signals * n_pairs * 4, hipMemcpyHostToDevice));
        HIPCHK(h, hipMemcpy(h->pairs, phase_pairs, (size_t)n_pairs * 2 * 4, hipMemcpyHostToDevice));
        HIPCHK(h, hipMemcpy(h->valid, valid, (size_t)h->K.n_signals * n_pairs * 4, hipMemcpyHostToDevice));
        h->n_pairs = n_pairs;
    }
    launch_maxwave(h, st, (int)use_pressure);
    HIPCHK(h, hipGetLastError());
    return RS_OK;
}

extern "C" int rs_get_buffer(rs_handle h, int32_t which, void **dev_ptr, int64_t shape[4], int32_t *ndim, int32_t *dtype) {
    if (!h || which < 0 || which >= RS_BUF_COUNT) return RS_EINVAL;
    rs_buf_describe(h->bufs[which], dev_ptr, shape, ndim, dtype);
    return RS_OK;
}

extern "C" int rs_read_buffer(rs_handle h, int32_t which, void *host_dst, int64_t nbytes) {
    if (!h || which < 0 || which >= RS_BUF_COUNT || !host_dst) return RS_EINVAL;
    auto &B = h->bufs[which];
    if ((size_t)nbytes != B.bytes) { h->err = "rs_read_buffer: size mismatch"; return RS_EINVAL; }
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, wait_idle(h));
    HIPCHK(h, hipMemcpy(host_dst, B.ptr, B.bytes, hipMemcpyDeviceToHost));
    return RS_OK;
}

extern "C" int rs_stats(rs_handle h, int64_t *host_out) {
    if (!h) return RS_EINVAL;
    return rs_read_buffer(h, RS_BUF_STATS, host_out, (int64_t)h->n_envs * ST_N * 8);
}

struct Snapshot { std::vector<void *> ptrs; uint32_t seed = 0; };     // the seed: the speed factors are recomputed from (seed, env, trip) at every load
// state AND the observation buffers: re-running observe would advance Signal.waiting_times
static const int kSnapBufs[] = {RS_BUF_LANE_AGG, RS_BUF_DRQ_NORM, RS_BUF_PHASE, RS_BUF_MPLIGHT, RS_BUF_WAVE, RS_BUF_WAIT,
                                RS_BUF_WAIT_NORM, RS_BUF_PRESSURE, RS_BUF_QUEUE_SUM, RS_BUF_QUEUE_MAX, RS_BUF_DRQ_NORM_F16,
                                RS_BUF_ENV, RS_BUF_TLS, RS_BUF_VEH_POS, RS_BUF_VEH_SPEED, RS_BUF_VEH_ACCEL, RS_BUF_VEH_TLOSS,
                                RS_BUF_VEH_LANE, RS_BUF_VEH_TRIP, RS_BUF_VEH_CURSOR, RS_BUF_VEH_SWAIT, RS_BUF_VEH_RWAIT,
                                RS_BUF_VEH_DEPART, RS_BUF_VEH_OWNER, RS_BUF_VEH_SF, RS_BUF_VEH_WTOT, RS_BUF_TRIP_LOG, RS_BUF_STATS,
                                RS_BUF_DEP_NEXT, RS_BUF_VEH_COOP, RS_BUF_VEH_COOPLEAD, RS_BUF_ARRIVALS, RS_BUF_DEPARTURES, RS_BUF_MPLIGHT_FULL,
                                RS_BUF_LANE_ARRIVALS, RS_BUF_VEH_COOP_ODD, RS_BUF_VEH_COOPLEAD_ODD, RS_BUF_VEH_MAIL};
extern "C" int rs_snapshot(rs_handle h, void **snap) {
    if (!h || !snap) return RS_EINVAL;
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, wait_idle(h));
    Snapshot *S = new Snapshot();
    S->seed = h->P.seed;
    for (int b : kSnapBufs) {
        void *d = nullptr;
        if (h->bufs[b].bytes == 0) { S->ptrs.push_back(nullptr); continue; }
        if (hipMalloc(&d, h->bufs[b].bytes) != hipSuccess) { h->err = "rs_snapshot: hipMalloc failed"; rs_snapshot_free(h, S); return RS_ENOMEM; }
        S->ptrs.push_back(d);
        HIPCHK(h, hipMemcpy(d, h->bufs[b].ptr, h->bufs[b].bytes, hipMemcpyDeviceToDevice));
    }
    *snap = S;
    return RS_OK;
}
extern "C" int rs_restore(rs_handle h, const void *snap) {
    if (!h || !snap) return RS_EINVAL;
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, wait_idle(h));
    const Snapshot *S = (const Snapshot *)snap;
    size_t i = 0;
    for (int b : kSnapBufs) { if (h->bufs[b].bytes) HIPCHK(h, hipMemcpy(h->bufs[b].ptr, S->ptrs[i], h->bufs[b].bytes, hipMemcpyDeviceToDevice)); ++i; }
    h->P.seed = S->seed;        // the vehicles on the network keep the speed factors they were inserted with
    return RS_OK;
}
extern "C" void rs_snapshot_free(rs_handle h, void *snap) {
    if (!snap) return;
    Snapshot *S = (Snapshot *)snap;
    for (void *p : S->ptrs) (void)hipFree(p);
    delete S;
}

extern "C" int rs_timing(rs_handle h, int32_t enable) {
    if (!h) return RS_EINVAL;
    h->timing = enable != 0;
    return RS_OK;
}
extern "C" int rs_timing_read(rs_handle h, float *total_ms, int32_t *launches) {
    if (!h) return RS_EINVAL;
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipDeviceSynchronize());
    float tot = 0.0f;
    for (size_t i = 0; i < h->ev_used; ++i) {
        float ms = 0.0f;
        HIPCHK(h, hipEventElapsedTime(&ms, h->events[i].first, h->events[i].second));
        tot += ms;
    }
    if (total_ms) *total_ms = tot;
    if (launches) *launches = (int32_t)h->ev_used;
    h->ev_used = 0;
    return RS_OK;
}

extern "C" int rs_phase_profile(rs_handle h, int32_t enable, uint64_t *host_out16) {
    if (!h) return RS_EINVAL;
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipDeviceSynchronize());
    if (h->prof && host_out16) HIPCHK(h, hipMemcpy(host_out16, h->prof, 16 * 8, hipMemcpyDeviceToHost));
    if (enable && !h->prof) { int rc = dev_alloc(h, &h->prof, 16); if (rc) return rc; }
    if (h->prof) HIPCHK(h, hipMemset(h->prof, 0, 16 * 8));
    if (!enable) h->prof = nullptr;     // the allocation stays on the handle's free list
    return RS_OK;
}

extern "C" int rs_set_seed(rs_handle h, uint32_t seed) {
    if (!h) return RS_EINVAL;
    h->P.seed = seed;
    return RS_OK;
}

extern "C" int rs_info(rs_handle h, int32_t *n_envs, int32_t *block_threads, int32_t *lds_bytes, int32_t *max_lanes_per_signal) {
    if (!h) return RS_EINVAL;
    rs_info_describe(h->n_envs, h->block, h->lds, h->K.lmax, n_envs, block_threads, lds_bytes, max_lanes_per_signal);
    return RS_OK;
}


// ------------------------------------------------------------------------------------------------ fused IDQN policy
enum { POLICY_IDQN = 0, POLICY_MPLIGHT = 1 };
struct rs_policy {
    int device = 0;
    int kind = POLICY_IDQN;     // which rs_*_create made it: the entry points of the other kind refuse it
    PolicyTab W{};              // IDQN
    FrapTab F{};                // MPLight
    std::vector<void *> allocs;
};

// what the two rs_*_create functions begin with: the result cleared, the number of visible devices
static int policy_devices(rs_policy_handle *out, int *ndev) {
    if (!out) return RS_EINVAL;
    *out = nullptr;
    if (hipGetDeviceCount(ndev) != hipSuccess || *ndev <= 0) { g_create_err = "no HIP device visible (this library has no CPU fallback)"; return RS_EHIP; }
    return RS_OK;
}
// ... and what they do once the arguments are checked: an empty policy of `kind` on the device, which is made current
static int policy_new(int device_id, int kind, rs_policy **p) {
    if (hipSetDevice(device_id) != hipSuccess) { g_create_err = "hipSetDevice failed"; return RS_EHIP; }
    *p = new (std::nothrow) rs_policy();
    if (!*p) return RS_ENOMEM;
    (*p)->device = device_id; (*p)->kind = kind;
    return RS_OK;
}
static void policy_destroy(rs_policy *p) {
    if (!p) return;
    (void)hipSetDevice(p->device);
    (void)hipDeviceSynchronize();
    for (void *d : p->allocs) (void)hipFree(d);
    delete p;
}
extern "C" void rs_idqn_destroy(rs_policy_handle p) { policy_destroy(p); }
extern "C" void rs_mplight_destroy(rs_policy_handle p) { policy_destroy(p); }

template <class T> static int pol_upload(rs_policy *p, const T **dst, const void *src, size_t count) {
    void *d = nullptr;
    if (hipMalloc(&d, count * sizeof(T) + 2048) != hipSuccess) return RS_ENOMEM;     // the fc1 copy passes may read up to 1 KB past the end
    p->allocs.push_back(d);
    if (hipMemcpy(d, src, count * sizeof(T), hipMemcpyHostToDevice) != hipSuccess) return RS_EHIP;
    *dst = (const T *)d;
    return RS_OK;
}

extern "C" int rs_idqn_create(int32_t device_id, int32_t n_signals, int32_t lmax, const int32_t *n_actions, const float *conv_w,
                              const float *conv_b, const uint16_t *w1, const float *b1, const uint16_t *w2, const float *b2,
                              const uint16_t *w3, const float *b3, rs_policy_handle *out) {
    int ndev = 0;
    if (int rc = policy_devices(out, &ndev)) return rc;
    if (device_id < 0 || device_id >= ndev || n_signals <= 0 || lmax < 2 || lmax > 17 || !n_actions || !conv_w || !conv_b || !w1 || !b1 || !w2 || !b2 || !w3 || !b3) {
        g_create_err = "rs_idqn_create: bad argument (1 <= signals, 2 <= lmax <= 17)"; return RS_EINVAL;
    }
    for (int s = 0; s < n_signals; ++s)
        if (n_actions[s] < 1 || n_actions[s] > POL_QMAX) { g_create_err = "rs_idqn_create: 1..8 actions per signal"; return RS_ELIMIT; }
    rs_policy *p = nullptr;
    int rc = policy_new(device_id, POLICY_IDQN, &p);
    if (rc) return rc;
    const size_t S = (size_t)n_signals, hp = (size_t)(lmax / 2);       // ceil((lmax - 1) / 2)
    p->W.S = n_signals; p->W.lmax = lmax; p->W.hp = (int32_t)hp;
    if ((rc = pol_upload<float>(p, &p->W.conv_w, conv_w, S * 64 * 4)) || (rc = pol_upload<float>(p, &p->W.conv_b, conv_b, S * 64)) ||
        (rc = pol_upload<h4_t>(p, &p->W.w1, w1, S * 64 * hp * 2 * 64)) || (rc = pol_upload<float>(p, &p->W.b1, b1, S * 64)) ||
        (rc = pol_upload<h4_t>(p, &p->W.w2, w2, S * 8 * 2 * 64)) || (rc = pol_upload<float>(p, &p->W.b2, b2, S * 64)) ||
        (rc = pol_upload<h4_t>(p, &p->W.w3, w3, S * 8 * 64)) || (rc = pol_upload<float>(p, &p->W.b3, b3, S * 32)) ||
        (rc = pol_upload<int32_t>(p, &p->W.n_actions, n_actions, S)) ||
        (rc = pol_upload<int32_t>(p, &p->W.hp_sig, std::vector<int32_t>(S, (int32_t)hp).data(), S))) {    // every k-step until rs_idqn_set_lanes says otherwise
        g_create_err = "rs_idqn_create: device allocation / upload failed";
        rs_idqn_destroy(p);
        return rc;
    }
    *out = p;
    return RS_OK;
}

static void idqn_launch(const PolicyTab &W, const void *obs, int n_envs, int env_base, int mode, float eps, uint32_t seed, uint32_t step_key,
                        const void *dyn, int32_t *actions, float *q, hipStream_t st) {
    hipLaunchKernelGGL(rs_idqn_forward_kernel, dim3((n_envs + POL_TM - 1) / POL_TM, W.S), dim3(256), 0, st, W, (const __half *)obs, n_envs, env_base,
                       mode, eps, seed, step_key, (const uint32_t *)dyn, actions, q);
}

extern "C" int rs_idqn_act(rs_policy_handle p, const void *obs, int32_t n_envs, int32_t env_base, int32_t mode, float epsilon, uint32_t seed, uint32_t step_key,
                           const void *dyn, int32_t *actions, float *q, void *stream) {
    if (!p || p->kind != POLICY_IDQN || !obs || !actions || n_envs <= 0 || mode < 0 || mode > 1) return RS_EINVAL;
    if (hipSetDevice(p->device) != hipSuccess) return RS_EHIP;
    idqn_launch(p->W, obs, n_envs, env_base, mode, epsilon, seed, step_key, dyn, actions, q, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? RS_OK : RS_EHIP;
}

// ---- IPPO: the actor-critic launch of the same trunk (resco_policy.h: rs_ippo_forward_kernel)
static void ippo_launch(const PolicyTab &W, const void *obs, int n_envs, int env_base, uint32_t seed, uint32_t step_key, const void *dyn,
                        int32_t *actions, int32_t *act2, float *logp, float *value, float *logits, hipStream_t st) {
    hipLaunchKernelGGL(rs_ippo_forward_kernel, dim3((n_envs + POL_TM - 1) / POL_TM, W.S), dim3(256), 0, st, W, (const __half *)obs, n_envs, env_base,
                       seed, step_key, (const uint32_t *)dyn, actions, logits, PolicyAC{act2, logp, value});
}

extern "C" int rs_ippo_act(rs_policy_handle p, const void *obs, int32_t n_envs, int32_t env_base, uint32_t seed, uint32_t step_key,
                           const void *dyn, int32_t *actions, float *logp, float *value, float *logits, void *stream) {
    // actions and logp come together, or not at all (value-only: the bootstrap value of the state after a segment)
    if (!p || p->kind != POLICY_IDQN || !obs || !value || n_envs <= 0 || (actions == nullptr) != (logp == nullptr)) return RS_EINVAL;
    if (hipSetDevice(p->device) != hipSuccess) return RS_EHIP;
    ippo_launch(p->W, obs, n_envs, env_base, seed, step_key, dyn, actions, nullptr, logp, value, logits, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? RS_OK : RS_EHIP;
}

// ---- PPO: GAE + per-signal standardisation (resco_ppo.h)
extern "C" int rs_ppo_gae(const float *rew, const float *value, const float *last_value, const uint8_t *done, int32_t T, int32_t n_envs,
                          int32_t n_signals, float gamma, float lambda, float *adv, float *ret, void *scratch, void *stream) {
    if (!rew || !value || !last_value || !done || !adv || !ret || !scratch || T <= 0 || n_envs <= 0 || n_signals <= 0) return RS_EINVAL;
    const PpoArgs A{rew, value, last_value, done, T, n_envs, n_signals, gamma, lambda, adv, ret, (float *)scratch};
    const int C = n_envs * n_signals;
    hipLaunchKernelGGL(rs_ppo_gae_columns_kernel, dim3((C + 255) / 256), dim3(256), 0, (hipStream_t)stream, A);
    hipLaunchKernelGGL(rs_ppo_standardise_kernel, dim3(n_signals), dim3(PPO_B), 0, (hipStream_t)stream, A);
    return hipGetLastError() == hipSuccess ? RS_OK : RS_EHIP;
}

// ---- The learner updates (resco_train.h).  What the handles of rs_ppo_create and rs_dqn_create share: the tensor sets are the
// caller's; the library owns the workspace and t.
struct TrainHandle {
    int device = 0;
    int max_batch = 0;          // the largest minibatch the workspace holds
    long long t = 0;            // Adam steps taken
    std::vector<void *> allocs;
    bool alloc(void **d, size_t bytes) {
        if (hipMalloc(d, bytes) != hipSuccess) return false;
        allocs.push_back(*d);
        return true;
    }
};
template <class Handle> static void train_destroy(Handle *p) {
    if (!p) return;
    (void)hipSetDevice(p->device);
    (void)hipDeviceSynchronize();
    for (void *d : p->allocs) (void)hipFree(d);
    delete p;
}

// rs_ppo_tensors / rs_dqn_tensors are the first nt pointers of the PT_* order
static_assert(sizeof(rs_ppo_tensors) == PPT_NT * sizeof(float *) && sizeof(rs_dqn_tensors) == (PT_FC3_B + 1) * sizeof(float *), "tensor sets");
static bool train_tensors_complete(const void *set, int nt) {
    for (int i = 0; set && i < nt; ++i)
        if (!((float *const *)set)[i]) return false;
    return set != nullptr;
}
static PptTensors train_tensors(const void *set, int nt) {
    PptTensors t{};
    for (int i = 0; i < nt; ++i) t.p[i] = ((float *const *)set)[i];
    return t;
}

// What rs_ppo_create and rs_dqn_create share: the argument checks (`name` and the caller's wording of its limits go into the text),
// the handle, the common fields of its table and the common workspace; part_size = ppt_p_size(NH).  sets: the caller's tensor sets of
// nt pointers each, params first; the table's par is set, the caller sets the others.  own(p): the caller's own allocations.
template <class Handle, class Own>
static int train_create(const char *name, const char *limits, int32_t device_id, int32_t n_signals, int32_t lmax, const int32_t *lanes,
                        const int32_t *n_actions, int32_t amax, const void *cfg, std::initializer_list<const void *> sets, int nt, int32_t max_batch,
                        int part_size, Handle **out, Own own) {
    if (!out) return RS_EINVAL;
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { g_create_err = "no HIP device visible (this library has no CPU fallback)"; return RS_EHIP; }
    if (device_id < 0 || device_id >= ndev || n_signals <= 0 || lmax < 2 || lmax > 17 || amax < 1 || amax > PPT_AMAX || !lanes || !n_actions || !cfg ||
        max_batch < 1) {
        g_create_err = std::string(name) + ": bad argument (" + limits + ")"; return RS_EINVAL;
    }
    for (const void *set : sets)
        if (!train_tensors_complete(set, nt)) { g_create_err = std::string(name) + ": a tensor pointer is NULL"; return RS_EINVAL; }
    for (int s = 0; s < n_signals; ++s)
        if (lanes[s] < 2 || lanes[s] > lmax || n_actions[s] < 1 || n_actions[s] > amax) {
            g_create_err = std::string(name) + ": 2 <= lanes[s] <= lmax and 1 <= n_actions[s] <= amax"; return RS_EINVAL;
        }
    if (hipSetDevice(device_id) != hipSuccess) { g_create_err = "hipSetDevice failed"; return RS_EHIP; }
    Handle *p = new (std::nothrow) Handle();
    if (!p) return RS_ENOMEM;
    p->device = device_id; p->max_batch = max_batch;
    PptTab &T = p->T;
    T.S = n_signals; T.lmax = lmax; T.amax = amax; T.H = lmax - 1;
    T.par = train_tensors(*sets.begin(), nt);
    T.tiles_max = (max_batch + PPT_TM - 1) / PPT_TM;
    T.bpad_max = T.tiles_max * PPT_TM;
    T.chunks_max = (T.bpad_max + PPT_CH - 1) / PPT_CH;
    const size_t S = (size_t)n_signals, H = (size_t)T.H;
    void *d_lanes = nullptr, *d_act = nullptr;
    if (!p->alloc(&d_lanes, S * 4) || !p->alloc(&d_act, S * 4) || !p->alloc((void **)&T.dz1, S * T.bpad_max * 64 * sizeof(float)) ||
        !p->alloc((void **)&T.part, S * T.tiles_max * part_size * sizeof(float)) ||
        !p->alloc((void **)&T.pw1, (size_t)T.chunks_max * S * H * 256 * 64 * sizeof(float)) ||
        !p->alloc((void **)&T.pconv, (size_t)T.chunks_max * S * H * 64 * 5 * sizeof(float)) || !own(p) ||
        hipMemcpy(d_lanes, lanes, S * 4, hipMemcpyHostToDevice) != hipSuccess || hipMemcpy(d_act, n_actions, S * 4, hipMemcpyHostToDevice) != hipSuccess) {
        g_create_err = std::string(name) + ": device allocation / upload failed";
        (void)hipGetLastError();
        train_destroy(p);
        return RS_ENOMEM;
    }
    T.lanes = (const int32_t *)d_lanes; T.n_actions = (const int32_t *)d_act;
    *out = p;
    return RS_OK;
}

// ---- PPO: the update itself (resco_ppo_train.h), four tensor sets
struct rs_ppo : TrainHandle {
    PpoTrainTab T{};
    rs_ppo_config cfg{};
};

extern "C" void rs_ppo_destroy(rs_ppo_handle p) { train_destroy(p); }

extern "C" int rs_ppo_create(int32_t device_id, int32_t n_signals, int32_t lmax, const int32_t *lanes, const int32_t *n_actions, int32_t amax,
                             const rs_ppo_config *cfg, const rs_ppo_tensors *params, const rs_ppo_tensors *grads, const rs_ppo_tensors *m,
                             const rs_ppo_tensors *v, int32_t max_minibatch, rs_ppo_handle *out) {
    const int rc = train_create("rs_ppo_create", "1 <= signals, 2 <= lmax <= 17, 1 <= amax <= 8, 1 <= max_minibatch", device_id, n_signals, lmax, lanes,
                                n_actions, amax, cfg, {params, grads, m, v}, PPT_NT, max_minibatch, ppt_p_size(PPO_NH), out, [&](rs_ppo *p) {
        return p->alloc((void **)&p->T.sqpart, (size_t)n_signals * (p->T.H + 1) * 2 * sizeof(float));
    });
    if (rc != RS_OK) return rc;
    rs_ppo *p = *out;
    p->cfg = *cfg;
    PpoTrainTab &T = p->T;
    T.grad = train_tensors(grads, PPT_NT); T.m = train_tensors(m, PPT_NT); T.v = train_tensors(v, PPT_NT);
    T.hp = PpoHyper{(float)cfg->clip_eps, (float)cfg->entropy_coef, (float)cfg->value_coef};
    return RS_OK;
}

// the launches of one minibatch gradient; the arguments have been checked
static void ppo_grad_launch(const rs_ppo *p, const PpoBatch &D, float *loss_out, hipStream_t st) {
    const PpoTrainTab &T = p->T;
    const int tiles = (D.B + PPT_TM - 1) / PPT_TM, chunks = (tiles * PPT_TM + PPT_CH - 1) / PPT_CH;
    hipLaunchKernelGGL(ppo_fwd_bwd_kernel, dim3(tiles, T.S), dim3(PPT_T), 0, st, T, D);
    hipLaunchKernelGGL(ppo_fc1_bwd_kernel, dim3(T.H * 2, chunks, T.S), dim3(PPT_T), 0, st, T, D);
    hipLaunchKernelGGL(ppo_reduce_kernel, dim3(T.S, T.H + (ppt_n_small(PPO_NH) + PPT_T - 1) / PPT_T), dim3(PPT_T), 0, st, T, D.B, loss_out);
}
static void ppo_step_launch(rs_ppo *p, hipStream_t st) {
    const PpoTrainTab &T = p->T;
    const PpoStepConsts K = ppo_step_consts(p->cfg.lr, p->cfg.adam_eps, p->cfg.beta1, p->cfg.beta2, p->cfg.max_grad_norm, p->t + 1);
    hipLaunchKernelGGL(ppo_norm_kernel, dim3(T.S, T.H + 1), dim3(PPT_T), 0, st, T);
    hipLaunchKernelGGL(ppo_adam_kernel, dim3(T.S, T.H + 1), dim3(PPT_T), 0, st, T, K);
    if (hipPeekAtLastError() == hipSuccess) p->t += 1;      // a step that could not be launched is not counted
}

extern "C" int rs_ppo_grad(rs_ppo_handle p, const void *obs, const int32_t *act, const float *logp, const float *adv, const float *ret,
                           const int32_t *idx, int32_t B, float *loss_out, void *stream) {
    if (!p) { g_create_err = "rs_ppo_grad: NULL handle"; return RS_EINVAL; }
    if (!obs || !act || !logp || !adv || !ret || !idx) { g_create_err = "rs_ppo_grad: a data pointer is NULL"; return RS_EINVAL; }
    if (B < 1 || B > p->max_batch) { g_create_err = "rs_ppo_grad: need 1 <= B <= max_minibatch of rs_ppo_create"; return RS_EINVAL; }
    if (hipSetDevice(p->device) != hipSuccess) return RS_EHIP;
    ppo_grad_launch(p, PpoBatch{(const __half *)obs, act, logp, adv, ret, idx, B}, loss_out, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? RS_OK : RS_EHIP;
}

extern "C" int rs_ppo_step(rs_ppo_handle p, void *stream) {
    if (!p) { g_create_err = "rs_ppo_step: NULL handle"; return RS_EINVAL; }
    if (hipSetDevice(p->device) != hipSuccess) return RS_EHIP;
    ppo_step_launch(p, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? RS_OK : RS_EHIP;
}

extern "C" int rs_ppo_fit(rs_ppo_handle p, const void *obs, const int32_t *act, const float *logp, const float *adv, const float *ret, int32_t n,
                          const int32_t *perm, int32_t epochs, int32_t minibatch, float *loss_out, void *stream) {
    if (!p) { g_create_err = "rs_ppo_fit: NULL handle"; return RS_EINVAL; }
    if (!obs || !act || !logp || !adv || !ret || !perm) { g_create_err = "rs_ppo_fit: a data pointer is NULL"; return RS_EINVAL; }
    if (n < 1 || epochs < 1 || minibatch < 1 || minibatch > p->max_batch) {
        g_create_err = "rs_ppo_fit: need 1 <= n, 1 <= epochs, 1 <= minibatch <= max_minibatch of rs_ppo_create"; return RS_EINVAL;
    }
    if (hipSetDevice(p->device) != hipSuccess) return RS_EHIP;
    for (int e = 0; e < epochs; ++e)
        for (int i = 0; i < n; i += minibatch) {
            const int B = n - i < minibatch ? n - i : minibatch;
            ppo_grad_launch(p, PpoBatch{(const __half *)obs, act, logp, adv, ret, perm + (size_t)e * n + i, B}, loss_out, (hipStream_t)stream);
            ppo_step_launch(p, (hipStream_t)stream);
        }
    return hipGetLastError() == hipSuccess ? RS_OK : RS_EHIP;
}

extern "C" int64_t rs_ppo_steps(rs_ppo_handle p) { return p ? (int64_t)p->t : -1; }

// ---- IDQN: the DQN update (resco_dqn_train.h), five tensor sets and the caller's ring; the library also owns the index array of
// rs_dqn_update
struct rs_dqn : TrainHandle {
    DqnTrainTab T{};
    rs_dqn_config cfg{};
    int32_t *idx = nullptr;     // [max_batch][S][2]: the minibatch rs_dqn_update draws
    const void *ring_ok[4] = {nullptr, nullptr, nullptr, nullptr};     // the ring arrays last found on this handle's device (dqn_check)
};

extern "C" void rs_dqn_destroy(rs_dqn_handle p) { train_destroy(p); }

extern "C" int rs_dqn_create(int32_t device_id, int32_t n_signals, int32_t lmax, const int32_t *lanes, const int32_t *n_actions, int32_t amax,
                             const rs_dqn_config *cfg, const rs_dqn_tensors *params, const rs_dqn_tensors *target, const rs_dqn_tensors *grads,
                             const rs_dqn_tensors *m, const rs_dqn_tensors *v, int32_t max_batch, rs_dqn_handle *out) {
    constexpr int NT = PT_FC3_B + 1;
    const int rc = train_create("rs_dqn_create", "a visible device, 1 <= signals, 2 <= lmax <= 17, 1 <= amax <= 8, 1 <= max_batch", device_id, n_signals, lmax,
                                lanes, n_actions, amax, cfg, {params, target, grads, m, v}, NT, max_batch, ppt_p_size(DQN_NH), out, [&](rs_dqn *p) {
        return p->alloc((void **)&p->T.y, (size_t)n_signals * p->T.bpad_max * sizeof(float)) &&
               p->alloc((void **)&p->idx, (size_t)max_batch * n_signals * 2 * sizeof(int32_t));
    });
    if (rc != RS_OK) return rc;
    rs_dqn *p = *out;
    p->cfg = *cfg;
    DqnTrainTab &T = p->T;
    T.tgt = train_tensors(target, NT); T.grad = train_tensors(grads, NT); T.m = train_tensors(m, NT); T.v = train_tensors(v, NT);
    T.gamma = (float)cfg->gamma;
    return RS_OK;
}

// what every call that reads the ring checks before it launches anything; `name` goes into the message
static bool dqn_on_device(const void *ptr, int device) {
    hipPointerAttribute_t at;
    if (hipPointerGetAttributes(&at, ptr) != hipSuccess) { (void)hipGetLastError(); return false; }     // (not memory the runtime knows)
    return at.device == device;
}
static int dqn_check(rs_dqn *p, const rs_dqn_ring *r, int32_t batch, const char *name) {
    auto refuse = [&](const char *why) { g_create_err = std::string(name) + ": " + why; return RS_EINVAL; };
    if (!p) return refuse("NULL handle");
    if (!r || !r->obs || !r->act || !r->rew || !r->done) return refuse("a ring pointer is NULL");
    if (batch < 1 || batch > p->max_batch) return refuse("need 1 <= batch <= max_batch of rs_dqn_create");
    if (r->capacity < 2 || r->n_envs < 1) return refuse("the ring needs capacity >= 2 and n_envs >= 1");
    if (r->count < 2) return refuse("the ring needs count >= 2: a transition is a slot and its written successor");
    if (r->count > r->capacity || r->head < 0 || r->head >= r->capacity) return refuse("head or count outside the ring");
    // where the four arrays live is asked of the runtime once per ring, not once per step: a ring keeps its storages
    const void *ring[4] = {r->obs, r->act, r->rew, r->done};
    if (memcmp(ring, p->ring_ok, sizeof(ring)) != 0) {
        for (const void *a : ring)
            if (!dqn_on_device(a, p->device)) return refuse("a ring array is not device memory of this handle's device (another device, or host memory)");
        memcpy(p->ring_ok, ring, sizeof(ring));
    }
    return RS_OK;
}
static DqnBatch dqn_batch(const rs_dqn_ring *r, const int32_t *idx, int32_t B) {
    return DqnBatch{(const __half *)r->obs, r->act, r->rew, r->done, r->capacity, r->n_envs, idx, B};
}

// the launches; the arguments have been checked
static void dqn_sample_launch(const rs_dqn *p, const rs_dqn_ring *r, int B, uint32_t seed, uint32_t key, int32_t *idx, hipStream_t st) {
    hipLaunchKernelGGL(dqn_sample_kernel, dim3((B * p->T.S + PPT_T - 1) / PPT_T), dim3(PPT_T), 0, st, seed, key, p->T.S, r->capacity, r->n_envs, r->head,
                       r->count, B, idx);
}
static void dqn_grad_launch(const rs_dqn *p, const DqnBatch &D, float *loss_out, hipStream_t st) {
    const DqnTrainTab &T = p->T;
    const int tiles = (D.B + PPT_TM - 1) / PPT_TM, chunks = (tiles * PPT_TM + PPT_CH - 1) / PPT_CH;
    hipLaunchKernelGGL(dqn_target_kernel, dim3(tiles, T.S), dim3(PPT_T), 0, st, T, D);
    hipLaunchKernelGGL(dqn_fwd_bwd_kernel, dim3(tiles, T.S), dim3(PPT_T), 0, st, T, D);
    hipLaunchKernelGGL(dqn_fc1_bwd_kernel, dim3(T.H * 2, chunks, T.S), dim3(PPT_T), 0, st, T, D);
    hipLaunchKernelGGL(dqn_reduce_kernel, dim3(T.S, T.H + (ppt_n_small(DQN_NH) + PPT_T - 1) / PPT_T), dim3(PPT_T), 0, st, T, D.B, loss_out);
}
static void dqn_step_launch(rs_dqn *p, hipStream_t st) {
    const PpoStepConsts K = ppo_step_consts(p->cfg.lr, p->cfg.adam_eps, p->cfg.beta1, p->cfg.beta2, 0.0, p->t + 1);
    hipLaunchKernelGGL(dqn_adam_kernel, dim3(p->T.S, p->T.H + 1), dim3(PPT_T), 0, st, p->T, K);
    if (hipPeekAtLastError() == hipSuccess) p->t += 1;      // a step that could not be launched is not counted
}

extern "C" int rs_dqn_sample(rs_dqn_handle p, const rs_dqn_ring *ring, int32_t batch, uint32_t seed, uint32_t update_key, int32_t *idx_out, void *stream) {
    if (int rc = dqn_check(p, ring, batch, "rs_dqn_sample")) return rc;
    if (!idx_out) { g_create_err = "rs_dqn_sample: idx_out is NULL"; return RS_EINVAL; }
    if (!dqn_on_device(idx_out, p->device)) { g_create_err = "rs_dqn_sample: idx_out is not device memory of this handle's device"; return RS_EINVAL; }
    if (hipSetDevice(p->device) != hipSuccess) return RS_EHIP;
    dqn_sample_launch(p, ring, batch, seed, update_key, idx_out, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? RS_OK : RS_EHIP;
}

extern "C" int rs_dqn_grad(rs_dqn_handle p, const rs_dqn_ring *ring, const int32_t *idx, int32_t batch, float *loss_out, void *stream) {
    if (int rc = dqn_check(p, ring, batch, "rs_dqn_grad")) return rc;
    if (!idx) { g_create_err = "rs_dqn_grad: idx is NULL"; return RS_EINVAL; }
    if (!dqn_on_device(idx, p->device)) { g_create_err = "rs_dqn_grad: idx is not device memory of this handle's device"; return RS_EINVAL; }
    if (hipSetDevice(p->device) != hipSuccess) return RS_EHIP;
    dqn_grad_launch(p, dqn_batch(ring, idx, batch), loss_out, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? RS_OK : RS_EHIP;
}

extern "C" int rs_dqn_step(rs_dqn_handle p, void *stream) {
    if (!p) { g_create_err = "rs_dqn_step: NULL handle"; return RS_EINVAL; }
    if (hipSetDevice(p->device) != hipSuccess) return RS_EHIP;
    dqn_step_launch(p, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? RS_OK : RS_EHIP;
}

extern "C" int rs_dqn_update(rs_dqn_handle p, const rs_dqn_ring *ring, int32_t batch, uint32_t seed, int32_t n_updates, float *loss_out, void *stream) {
    if (int rc = dqn_check(p, ring, batch, "rs_dqn_update")) return rc;
    if (n_updates < 1) { g_create_err = "rs_dqn_update: need 1 <= n_updates"; return RS_EINVAL; }
    if (hipSetDevice(p->device) != hipSuccess) return RS_EHIP;
    for (int j = 0; j < n_updates; ++j) {       // the launches of a stream run in order: update j + 1 may overwrite idx and the workspace
        dqn_sample_launch(p, ring, batch, seed, (uint32_t)p->t, p->idx, (hipStream_t)stream);
        dqn_grad_launch(p, dqn_batch(ring, p->idx, batch), loss_out, (hipStream_t)stream);
        dqn_step_launch(p, (hipStream_t)stream);
        if (hipPeekAtLastError() != hipSuccess) break;      // nothing more is enqueued behind a launch that failed
    }
    return hipGetLastError() == hipSuccess ? RS_OK : RS_EHIP;
}

extern "C" int64_t rs_dqn_steps(rs_dqn_handle p) { return p ? (int64_t)p->t : -1; }

// ------------------------------------------------------------------------------------------------ fused MPLight (FRAP) policy
static void mplight_launch(const FrapTab &F, const void *obs, int n_envs, int env_base, float eps, uint32_t seed, uint32_t step_key,
                           const void *dyn, int32_t *actions, int32_t *pair_out, float *q, hipStream_t st) {
    const int G = F.P <= 4 ? 4 : (F.P <= 8 ? 8 : 16), rows = 256 / G;
    hipLaunchKernelGGL(rs_mplight_act_kernel, dim3((n_envs + rows - 1) / rows, F.S), dim3(256), 0, st, F, obs, n_envs, env_base, eps, seed,
                       step_key, (const uint32_t *)dyn, actions, pair_out, q);
}

extern "C" int rs_mplight_create(int32_t device_id, int32_t demand_shape, int32_t n_pairs, const int32_t *pairs, int32_t n_signals,
                                 const int32_t *valid, const int32_t *order, const float *weights, rs_policy_handle *out) {
    int ndev = 0;
    if (int rc = policy_devices(out, &ndev)) return rc;
    if (device_id < 0 || device_id >= ndev || (demand_shape != 1 && demand_shape != 4) || n_pairs < 2 || n_pairs > FRAP_PMAX || n_signals <= 0 ||
        !pairs || !valid || !order || !weights) {
        g_create_err = "rs_mplight_create: bad argument (demand_shape 1 or 4, 2 <= n_pairs <= 16, 1 <= n_signals, tables and weights required)";
        return RS_EINVAL;
    }
    const int P = n_pairs, S = n_signals;
    for (int i = 0; i < 2 * P; ++i)
        if (pairs[i] < 0 || pairs[i] >= FRAP_MV) { g_create_err = "rs_mplight_create: a phase pair names a movement outside 0..11"; return RS_EINVAL; }
    // the exploration draw takes the k-th valid pair of the dict order; the reference takes reverse_valid[k]: the same pair only while
    // the local actions of the valid pairs, in dict order, are 0, 1, .., n - 1
    std::vector<int32_t> nv((size_t)S, 0);
    for (int s = 0; s < S; ++s) {
        int n = 0;
        while (n < P && order[s * P + n] >= 0) ++n;
        int n_valid = 0;
        for (int g = 0; g < P; ++g) n_valid += valid[s * P + g] >= 0;
        if (n == 0 || n != n_valid) { g_create_err = "rs_mplight_create: order[s] must list exactly the valid pairs of signal s (at least one)"; return RS_EINVAL; }
        for (int k = 0; k < n; ++k) {
            const int g = order[s * P + k];
            if (g >= P || valid[s * P + g] != k) {
                g_create_err = "rs_mplight_create: the local actions of a signal's valid pairs, in dict order, must be 0 .. n-1"; return RS_EINVAL; }
        }
        nv[(size_t)s] = n;
    }
    rs_policy *p = nullptr;
    int rc = policy_new(device_id, POLICY_MPLIGHT, &p);
    if (rc) return rc;
    p->F.P = P; p->F.S = S; p->F.D = demand_shape;
    const size_t nw = (size_t)FrapOff(demand_shape).n;
    if ((rc = pol_upload<float>(p, &p->F.w, weights, nw)) || (rc = pol_upload<int32_t>(p, &p->F.pairs, pairs, (size_t)P * 2)) ||
        (rc = pol_upload<int32_t>(p, &p->F.valid, valid, (size_t)S * P)) || (rc = pol_upload<int32_t>(p, &p->F.order, order, (size_t)S * P)) ||
        (rc = pol_upload<int32_t>(p, &p->F.nvalid, nv.data(), (size_t)S))) {
        g_create_err = "rs_mplight_create: device allocation / upload failed";
        rs_mplight_destroy(p);
        return rc;
    }
    *out = p;
    return RS_OK;
}

extern "C" int rs_mplight_act(rs_policy_handle p, const void *obs, int32_t n_envs, int32_t env_base, float epsilon, uint32_t seed, uint32_t step_key,
                              const void *dyn, int32_t *actions, int32_t *pair_index, float *q, void *stream) {
    if (!p || p->kind != POLICY_MPLIGHT || !obs || !actions || n_envs <= 0) return RS_EINVAL;
    if (hipSetDevice(p->device) != hipSuccess) return RS_EHIP;
    mplight_launch(p->F, obs, n_envs, env_base, epsilon, seed, step_key, dyn, actions, pair_index, q, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? RS_OK : RS_EHIP;
}

extern "C" int rs_mplight_set_device_weights(rs_policy_handle p, const float *weights) {
    if (!p || p->kind != POLICY_MPLIGHT || !weights) return RS_EINVAL;
    p->F.w = weights;
    return RS_OK;
}

// ---- MPLight: the shared-DQN update (resco_frap_train.h), five flat vectors and the caller's ring; the library owns the per-tile
// partials, the pair table and the index array of rs_mplight_dqn_update
struct rs_mplight_dqn : TrainHandle {
    FrapTrainTab T{};
    rs_dqn_config cfg{};
    int32_t *idx = nullptr;     // [max_batch][3]: the minibatch rs_mplight_dqn_update draws
    const void *ring_ok[4] = {nullptr, nullptr, nullptr, nullptr};     // the ring arrays last found on this handle's device
};

extern "C" void rs_mplight_dqn_destroy(rs_mplight_dqn_handle p) { train_destroy(p); }

extern "C" int rs_mplight_dqn_create(int32_t device_id, int32_t demand_shape, int32_t n_pairs, const int32_t *pairs, int32_t n_signals,
                                     const rs_dqn_config *cfg, float *params, const float *target, float *grads, float *m, float *v, int32_t max_batch,
                                     rs_mplight_dqn_handle *out) {
    if (!out) return RS_EINVAL;
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { g_create_err = "no HIP device visible (this library has no CPU fallback)"; return RS_EHIP; }
    if (device_id < 0 || device_id >= ndev || (demand_shape != 1 && demand_shape != 4) || n_pairs < 2 || n_pairs > FRAP_PMAX || n_signals < 1 || !pairs ||
        !cfg || max_batch < 1) {
        g_create_err = "rs_mplight_dqn_create: bad argument (a visible device, demand_shape 1 or 4, 2 <= n_pairs <= 16, 1 <= n_signals, 1 <= max_batch)";
        return RS_EINVAL;
    }
    if (!params || !target || !grads || !m || !v) { g_create_err = "rs_mplight_dqn_create: a vector pointer is NULL"; return RS_EINVAL; }
    for (int i = 0; i < 2 * n_pairs; ++i)
        if (pairs[i] < 0 || pairs[i] >= FRAP_MV) { g_create_err = "rs_mplight_dqn_create: a phase pair names a movement outside 0..11"; return RS_EINVAL; }
    if (hipSetDevice(device_id) != hipSuccess) { g_create_err = "hipSetDevice failed"; return RS_EHIP; }
    rs_mplight_dqn *p = new (std::nothrow) rs_mplight_dqn();
    if (!p) return RS_ENOMEM;
    p->device = device_id; p->max_batch = max_batch; p->cfg = *cfg;
    FrapTrainTab &T = p->T;
    T.par = params; T.tgt = target; T.grad = grads; T.m = m; T.v = v;
    T.P = n_pairs; T.D = demand_shape; T.S = n_signals; T.n = FrapOff(demand_shape).n;
    T.tiles_max = (max_batch + FPT_TM - 1) / FPT_TM;
    T.gamma = cfg->gamma;
    void *d_pairs = nullptr;
    if (!p->alloc(&d_pairs, (size_t)n_pairs * 2 * 4) || !p->alloc((void **)&T.part, (size_t)T.tiles_max * FG_N * sizeof(fpt_t)) ||
        !p->alloc((void **)&p->idx, (size_t)max_batch * 3 * sizeof(int32_t)) ||
        hipMemcpy(d_pairs, pairs, (size_t)n_pairs * 2 * 4, hipMemcpyHostToDevice) != hipSuccess) {
        g_create_err = "rs_mplight_dqn_create: device allocation / upload failed";
        (void)hipGetLastError();
        train_destroy(p);
        return RS_ENOMEM;
    }
    T.pairs = (const int32_t *)d_pairs;
    *out = p;
    return RS_OK;
}

// what every call that reads the ring checks before it launches anything; `name` goes into the message
static int mplight_dqn_check(rs_mplight_dqn *p, const rs_mplight_ring *r, int32_t batch, const char *name) {
    auto refuse = [&](const char *why) { g_create_err = std::string(name) + ": " + why; return RS_EINVAL; };
    if (!p) return refuse("NULL handle");
    if (!r || !r->obs || !r->act || !r->rew || !r->done) return refuse("a ring pointer is NULL");
    if (batch < 1 || batch > p->max_batch) return refuse("need 1 <= batch <= max_batch of rs_mplight_dqn_create");
    if (r->capacity < 2 || r->n_envs < 1) return refuse("the ring needs capacity >= 2 and n_envs >= 1");
    if (r->n_signals != p->T.S) return refuse("the ring's n_signals is not the handle's");
    if (r->width != 1 + FRAP_MV * p->T.D) return refuse("the ring's width is not the handle's 1 + 12 demand_shape");
    if (r->count < 2) return refuse("the ring needs count >= 2: a transition is a slot and its written successor");
    if (r->count > r->capacity || r->head < 0 || r->head >= r->capacity) return refuse("head or count outside the ring");
    const void *ring[4] = {r->obs, r->act, r->rew, r->done};      // asked of the runtime once per ring: a ring keeps its storages
    if (memcmp(ring, p->ring_ok, sizeof(ring)) != 0) {
        for (const void *a : ring)
            if (!dqn_on_device(a, p->device)) return refuse("a ring array is not device memory of this handle's device (another device, or host memory)");
        memcpy(p->ring_ok, ring, sizeof(ring));
    }
    return RS_OK;
}
static FrapBatch mplight_dqn_batch(const rs_mplight_ring *r, const int32_t *idx, int32_t B) {
    return FrapBatch{r->obs, r->act, r->rew, r->done, r->capacity, r->n_envs, r->n_signals, r->width, idx, B};
}

// the launches; the arguments have been checked
static void mplight_dqn_sample_launch(const rs_mplight_ring *r, int B, uint32_t seed, uint32_t key, int32_t *idx, hipStream_t st) {
    hipLaunchKernelGGL(frap_dqn_sample_kernel, dim3((B + 255) / 256), dim3(256), 0, st, seed, key, r->capacity, r->n_envs, r->n_signals, r->head, r->count, B,
                       idx);
}
static void mplight_dqn_grad_launch(const rs_mplight_dqn *p, const FrapBatch &D, float *loss_out, hipStream_t st) {
    const FrapTrainTab &T = p->T;
    hipLaunchKernelGGL(frap_dqn_tile_kernel, dim3((D.B + FPT_TM - 1) / FPT_TM), dim3(FPT_T), 0, st, T, D);
    hipLaunchKernelGGL(frap_dqn_reduce_kernel, dim3((T.n + 255) / 256), dim3(256), 0, st, T, D.B, loss_out);
}
static void mplight_dqn_step_launch(rs_mplight_dqn *p, hipStream_t st) {
    const PpoStepConsts K = ppo_step_consts(p->cfg.lr, p->cfg.adam_eps, p->cfg.beta1, p->cfg.beta2, 0.0, p->t + 1);
    hipLaunchKernelGGL(frap_dqn_adam_kernel, dim3((p->T.n + 255) / 256), dim3(256), 0, st, p->T, K);
    if (hipPeekAtLastError() == hipSuccess) p->t += 1;      // a step that could not be launched is not counted
}

extern "C" int rs_mplight_dqn_sample(rs_mplight_dqn_handle p, const rs_mplight_ring *ring, int32_t batch, uint32_t seed, uint32_t update_key,
                                     int32_t *idx_out, void *stream) {
    if (int rc = mplight_dqn_check(p, ring, batch, "rs_mplight_dqn_sample")) return rc;
    if (!idx_out) { g_create_err = "rs_mplight_dqn_sample: idx_out is NULL"; return RS_EINVAL; }
    if (!dqn_on_device(idx_out, p->device)) { g_create_err = "rs_mplight_dqn_sample: idx_out is not device memory of this handle's device"; return RS_EINVAL; }
    if (hipSetDevice(p->device) != hipSuccess) return RS_EHIP;
    mplight_dqn_sample_launch(ring, batch, seed, update_key, idx_out, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? RS_OK : RS_EHIP;
}

extern "C" int rs_mplight_dqn_grad(rs_mplight_dqn_handle p, const rs_mplight_ring *ring, const int32_t *idx, int32_t batch, float *loss_out, void *stream) {
    if (int rc = mplight_dqn_check(p, ring, batch, "rs_mplight_dqn_grad")) return rc;
    if (!idx) { g_create_err = "rs_mplight_dqn_grad: idx is NULL"; return RS_EINVAL; }
    if (!dqn_on_device(idx, p->device)) { g_create_err = "rs_mplight_dqn_grad: idx is not device memory of this handle's device"; return RS_EINVAL; }
    if (hipSetDevice(p->device) != hipSuccess) return RS_EHIP;
    mplight_dqn_grad_launch(p, mplight_dqn_batch(ring, idx, batch), loss_out, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? RS_OK : RS_EHIP;
}

extern "C" int rs_mplight_dqn_step(rs_mplight_dqn_handle p, void *stream) {
    if (!p) { g_create_err = "rs_mplight_dqn_step: NULL handle"; return RS_EINVAL; }
    if (hipSetDevice(p->device) != hipSuccess) return RS_EHIP;
    mplight_dqn_step_launch(p, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? RS_OK : RS_EHIP;
}

extern "C" int rs_mplight_dqn_update(rs_mplight_dqn_handle p, const rs_mplight_ring *ring, int32_t batch, uint32_t seed, int32_t n_updates, float *loss_out,
                                     void *stream) {
    if (int rc = mplight_dqn_check(p, ring, batch, "rs_mplight_dqn_update")) return rc;
    if (n_updates < 1) { g_create_err = "rs_mplight_dqn_update: need 1 <= n_updates"; return RS_EINVAL; }
    if (hipSetDevice(p->device) != hipSuccess) return RS_EHIP;
    for (int j = 0; j < n_updates; ++j) {       // the launches of a stream run in order: update j + 1 may overwrite idx and the workspace
        mplight_dqn_sample_launch(ring, batch, seed, (uint32_t)p->t, p->idx, (hipStream_t)stream);
        mplight_dqn_grad_launch(p, mplight_dqn_batch(ring, p->idx, batch), loss_out, (hipStream_t)stream);
        mplight_dqn_step_launch(p, (hipStream_t)stream);
        if (hipPeekAtLastError() != hipSuccess) break;      // nothing more is enqueued behind a launch that failed
    }
    return hipGetLastError() == hipSuccess ? RS_OK : RS_EHIP;
}

extern "C" int64_t rs_mplight_dqn_steps(rs_mplight_dqn_handle p) { return p ? (int64_t)p->t : -1; }

// ---- one env-step (or n of them) of a whole group of handles in ONE call (include/resco_sim.h: rs_group_step)
extern "C" int rs_group_step(const rs_handle *hs, int32_t n_handles, const rs_group_agent *agent, int32_t n_steps) {
    if (!hs || n_handles <= 0 || n_steps <= 0) return RS_EINVAL;
    const int kind = agent ? agent->kind : RS_AGENT_NONE;
    for (int i = 0; i < n_handles; ++i) {
        rs_sim *h = hs[i];
        if (!h) return RS_EINVAL;
        if (kind == RS_AGENT_MAXWAVE || kind == RS_AGENT_MAXPRESSURE) {
            if (!h->pairs) { h->err = "rs_group_step: the MAXWAVE / MAXPRESSURE tables are installed by a first rs_act_maxwave call"; return RS_EINVAL; }
            if (!(h->out_mask & (kind == RS_AGENT_MAXPRESSURE ? OUT_MPLIGHT : OUT_WAVE))) { h->err = "rs_group_step: the agent's input buffer is switched off (rs_set_outputs)"; return RS_EINVAL; }
        } else if (kind == RS_AGENT_IDQN) {
            if (!agent->policy || agent->policy->kind != POLICY_IDQN || agent->mode < 0 || agent->mode > 1 || agent->policy->W.S != h->K.n_signals || agent->policy->W.lmax != h->K.lmax) {
                h->err = "rs_group_step: RS_AGENT_IDQN needs a policy built for this scenario (n_signals, lmax)"; return RS_EINVAL; }
            if (agent->policy->device != h->device) { h->err = "rs_group_step: the policy's weights live on another device than this handle"; return RS_EINVAL; }
            if (!(h->out_mask & OUT_DRQ_F16)) { h->err = "rs_group_step: RS_AGENT_IDQN reads RS_BUF_DRQ_NORM_F16, which rs_set_outputs has switched off"; return RS_EINVAL; }
        } else if (kind == RS_AGENT_MPLIGHT) {
            if (!agent->policy || agent->policy->kind != POLICY_MPLIGHT || agent->policy->F.S != h->K.n_signals) {
                h->err = "rs_group_step: RS_AGENT_MPLIGHT needs an rs_mplight_create policy built for this scenario (n_signals)"; return RS_EINVAL; }
            if (agent->mode != 0) { h->err = "rs_group_step: RS_AGENT_MPLIGHT has only mode 0 (epsilon-greedy)"; return RS_EINVAL; }
            if (agent->policy->device != h->device) { h->err = "rs_group_step: the policy's weights live on another device than this handle"; return RS_EINVAL; }
            if (!(h->out_mask & (agent->policy->F.D == 1 ? OUT_MPLIGHT : OUT_MPLIGHT_FULL))) {
                h->err = agent->policy->F.D == 1 ? "rs_group_step: RS_AGENT_MPLIGHT reads RS_BUF_MPLIGHT, which rs_set_outputs has switched off"
                                                 : "rs_group_step: RS_AGENT_MPLIGHT reads RS_BUF_MPLIGHT_FULL, which rs_set_outputs has switched off";
                return RS_EINVAL;
            }
        } else if (kind != RS_AGENT_NONE && kind != RS_AGENT_RANDOM) { h->err = "rs_group_step: unknown agent kind"; return RS_EINVAL; }
    }
    for (int k = 0; k < n_steps; ++k)
        for (int i = 0; i < n_handles; ++i) {
            rs_sim *h = hs[i];
            hipStream_t st;
            if (int rc = enter(h, nullptr, &st)) return rc;
            const uint32_t key = agent ? agent->step_key + (uint32_t)k : 0u;
            float eps = agent ? agent->epsilon + (float)k * agent->epsilon_step : 0.0f;
            if (eps < 0.0f) eps = 0.0f;
            if (kind == RS_AGENT_RANDOM) launch_random(h, st, key);
            else if (kind == RS_AGENT_MAXWAVE || kind == RS_AGENT_MAXPRESSURE) launch_maxwave(h, st, kind == RS_AGENT_MAXPRESSURE);
            else if (kind == RS_AGENT_IDQN)
                idqn_launch(agent->policy->W, h->O.drq_f16(), h->n_envs, h->P.env_base, agent->mode, eps, agent->seed, key, nullptr, h->actions, nullptr, st);
            else if (kind == RS_AGENT_MPLIGHT) {
                const FrapTab &F = agent->policy->F;
                const void *obs = F.D == 1 ? (const void *)h->O.mplight() : (const void *)h->O.mplight_full();
                mplight_launch(F, obs, h->n_envs, h->P.env_base, eps, agent->seed, key, nullptr, h->actions, nullptr, nullptr, st);
            }
            if (kind != RS_AGENT_NONE) HIPCHK(h, hipGetLastError());
            const int rc = launch_step(h, st, h->K.step_length * h->ratio, 1);
            if (rc != RS_OK) return rc;
        }
    return RS_OK;
}

// ---- rs_group_rollout: rs_group_step with the IPPO actor-critic kernel and a trajectory recorder (include/resco_sim.h)
// What a segment needs beside what the policy kernel writes itself (act, logp, value): the observation the policy saw and the reward
// after the step.  One small kernel AFTER every step kernel copies the reward into slot t and the new observation into slot t + 1
// (when this call records it); one more, before the first step, the first observation: n_steps + 1 launches beside the 2 n_steps of
// rs_group_step.  Measured against hipMemcpyAsync device-to-device on the stream (2 n_steps copies): the kernel is ~1 % faster on
// cologne1 x 256 and level on ingolstadt21 x 1024 x 2 pipes (profiles/r08_ippo_device_rollout.txt), so the copies are not built.
// rew: n_rew floats; obs: n_half halfs, as 16-byte words when `vec` (both pointers 16-byte aligned; the tail goes half by half),
// half by half otherwise; either source may be NULL.  Grid-stride loops: any grid covers any size.
__global__ void __launch_bounds__(256)
rs_rollout_record_kernel(const float *__restrict__ rew_src, float *__restrict__ rew_dst, int n_rew, const uint16_t *__restrict__ obs_src,
                         uint16_t *__restrict__ obs_dst, int n_half, int vec) {
    const int i0 = blockIdx.x * 256 + threadIdx.x, stride = gridDim.x * 256;
    if (rew_src)
        for (int i = i0; i < n_rew; i += stride) rew_dst[i] = rew_src[i];
    if (obs_src) {
        const int n8 = vec ? n_half >> 3 : 0;
        for (int i = i0; i < n8; i += stride) ((uint4 *)obs_dst)[i] = ((const uint4 *)obs_src)[i];
        for (int i = n8 * 8 + i0; i < n_half; i += stride) obs_dst[i] = obs_src[i];
    }
}

extern "C" int rs_group_rollout(const rs_handle *hs, int32_t n_handles, const rs_group_agent *agent, const rs_rollout *segs, int32_t t0, int32_t n_steps) {
    if (!hs || n_handles <= 0 || n_steps <= 0 || t0 < 0 || !segs) return RS_EINVAL;
    for (int i = 0; i < n_handles; ++i) {
        rs_sim *h = hs[i];
        if (!h) return RS_EINVAL;
        const rs_rollout &R = segs[i];
        if (!agent || agent->kind != RS_AGENT_IPPO) { h->err = "rs_group_rollout: the agent must be RS_AGENT_IPPO"; return RS_EINVAL; }
        if (!agent->policy || agent->policy->kind != POLICY_IDQN || agent->policy->W.S != h->K.n_signals || agent->policy->W.lmax != h->K.lmax) {
            h->err = "rs_group_rollout: RS_AGENT_IPPO needs an rs_idqn_create policy built for this scenario (n_signals, lmax)"; return RS_EINVAL; }
        if (agent->policy->device != h->device) { h->err = "rs_group_rollout: the policy's weights live on another device than this handle"; return RS_EINVAL; }
        if (!(h->out_mask & OUT_DRQ_F16)) { h->err = "rs_group_rollout: RS_AGENT_IPPO reads RS_BUF_DRQ_NORM_F16, which rs_set_outputs has switched off"; return RS_EINVAL; }
        if (!R.obs || !R.act || !R.logp || !R.value || !R.rew) { h->err = "rs_group_rollout: a segment buffer is NULL"; return RS_EINVAL; }
        if ((long long)t0 + n_steps > R.T) { h->err = "rs_group_rollout: t0 + n_steps exceeds the segment's T slots"; return RS_EINVAL; }
    }
    for (int k = 0; k < n_steps; ++k)
        for (int i = 0; i < n_handles; ++i) {
            rs_sim *h = hs[i];
            const rs_rollout &R = segs[i];
            hipStream_t st;
            if (int rc = enter(h, nullptr, &st)) return rc;
            const size_t ns = (size_t)h->n_envs * h->K.n_signals, no = ns * h->K.lmax * 5, t = (size_t)(t0 + k);
            const uint16_t *obs = h->O.drq_f16();
            uint16_t *obs_t = (uint16_t *)R.obs + t * no;
            const int vec = (((uintptr_t)obs | (uintptr_t)obs_t | (no * 2)) & 15) == 0;      // (no * 2: the next slot is aligned as well)
            const size_t items = vec ? (no / 8 > ns ? no / 8 : ns) : no;
            const int grid = (int)((items + 255) / 256);
            if (k == 0) hipLaunchKernelGGL(rs_rollout_record_kernel, dim3(grid), dim3(256), 0, st, nullptr, nullptr, 0, obs, obs_t, (int)no, vec);
            ippo_launch(agent->policy->W, obs, h->n_envs, h->P.env_base, agent->seed, agent->step_key + (uint32_t)k, nullptr, h->actions,
                        R.act + t * ns, R.logp + t * ns, R.value + t * ns, nullptr, st);
            HIPCHK(h, hipGetLastError());
            const int rc = launch_step(h, st, h->K.step_length * h->ratio, 1);
            if (rc != RS_OK) return rc;
            const bool next = k + 1 < n_steps;
            hipLaunchKernelGGL(rs_rollout_record_kernel, dim3(grid), dim3(256), 0, st, (const float *)h->O.wait_norm(), R.rew + t * ns, (int)ns,
                               next ? obs : nullptr, obs_t + no, (int)no, vec);
            HIPCHK(h, hipGetLastError());
        }
    return RS_OK;
}

extern "C" int rs_idqn_set_device_weights(rs_policy_handle p, const float *conv_w, const float *conv_b, const uint16_t *w1, const float *b1,
                                          const uint16_t *w2, const float *b2, const uint16_t *w3, const float *b3) {
    if (!p || p->kind != POLICY_IDQN) return RS_EINVAL;
    if (conv_w) p->W.conv_w = conv_w;
    if (conv_b) p->W.conv_b = conv_b;
    if (w1) p->W.w1 = (const h4_t *)w1;
    if (b1) p->W.b1 = b1;
    if (w2) p->W.w2 = (const h4_t *)w2;
    if (b2) p->W.b2 = b2;
    if (w3) p->W.w3 = (const h4_t *)w3;
    if (b3) p->W.b3 = b3;
    return RS_OK;
}

// The networks' own input sizes: signal s observes lanes[s] lanes, so the fc1 rows of its padded lanes (beyond (lanes[s] - 1) * 4
// per conv channel) are zero and the kernel may skip their k-steps -- results are unchanged, the work follows the real head sizes.
extern "C" int rs_idqn_set_lanes(rs_policy_handle p, const int32_t *lanes_per_signal) {
    if (!p || p->kind != POLICY_IDQN || !lanes_per_signal) return RS_EINVAL;
    if (hipSetDevice(p->device) != hipSuccess) return RS_EHIP;
    std::vector<int32_t> hp((size_t)p->W.S);
    for (int s = 0; s < p->W.S; ++s) {
        const int l = lanes_per_signal[s];
        if (l < 2 || l > p->W.lmax) { g_create_err = "rs_idqn_set_lanes: 2 <= lanes[s] <= lmax"; return RS_EINVAL; }
        hp[(size_t)s] = l / 2;                                  // ceil((l - 1) / 2)
    }
    if (hipDeviceSynchronize() != hipSuccess) return RS_EHIP;
    return hipMemcpy((void *)p->W.hp_sig, hp.data(), hp.size() * sizeof(int32_t), hipMemcpyHostToDevice) == hipSuccess ? RS_OK : RS_EHIP;
}
