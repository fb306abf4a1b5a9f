// Optimizer step of the training path as three multi-tensor launches over ALL parameters:
//   reference engine/trainer.py:614-622  optimizer_step: clip_grad_norm_(max_norm 10) -> SGD(nesterov) step -> EMA update
//   reference engine/trainer.py:788-849  build_optimizer: three parameter groups (biases / decayed weights / norm weights)
//   reference utils/torch_utils.py:657-673 ModelEMA.update: v = d*v + (1-d)*model value, d = decay*(1 - exp(-updates/tau))
//
//  1. ymi_opt_sumsq   : per-chunk sums of squares of every gradient           (reads g once)
//  2. (same call)     : fixed-order final sum -> total norm -> clip coefficient, update counter += 1, EMA decay
//  3. ymi_opt_update  : g*clip (+ wd*p) -> momentum buffer -> nesterov -> p -= lr*g -> ema  (one pass: p, g, buf, ema)
//     or, rule R_ADAMW / R_ADAM, torch.optim.AdamW / Adam (the reference's 'AdamW' / 'Adam' branches, trainer.py:829-830, which
//     'auto' picks for short runs, :812): decoupled decay p *= 1 - lr*wd (Adam: g += wd*p), m = lerp(m, g, 1-b1),
//     v = b2*v + (1-b2)*g*g, p -= lr/(1-b1^t) * m / (sqrt(v)/sqrt(1-b2^t) + eps); t counted on the device by pass 2.
//     R_ADAMAX .. R_RMSPROP: the remaining branches of build_optimizer (trainer.py:827-832) with torch's default hyper-parameters -
//     Adamax (exp_inf = max(b2*exp_inf, |g| + eps)), NAdam (Nesterov momentum schedule mu_t, its running product kept in the state),
//     RAdam (variance rectification once rho_t > 5), RMSprop(momentum) - each one straight-line body of the same pass.
//
// HBM-bound: 28 B per parameter (p, g, buf, ema read; p, buf, ema written; Adam: 36 B with the second moment).  No torch.stack / foreach chains: every
// operand is addressed through a device table built once (parameters, momentum and EMA buffers never move); the gradient
// tensors, whose addresses change from step to step in eager mode, travel by value in the kernel arguments, so the
// launches are graph-capturable without any host staging buffer.
// Hyper-parameters (per-group lr / weight decay, momentum, max norm, EMA decay and tau) live in a small device array the
// host rewrites only when a scheduler changes them: a replayed HIP graph follows the schedule.
#include <math.h>

#include "common.h"

namespace {
constexpr int OPT_CHUNK = 4096;  // elements per workgroup (256 threads x 4 float4)
constexpr int OPT_GRADS = YMI_OPT_MAX_GRADS;

struct GradPtrs {
    const float* g[OPT_GRADS];
};

// the update rules: ymi_opt_update's `rule`, hyper[H_RULE], the RULE of opt_update_kernel and engine/optim.py's RULE
enum Rule { R_SGD, R_ADAMW, R_ADAM, R_ADAMAX, R_NADAM, R_RADAM, R_RMSPROP, R_COUNT };

// hyper layout (floats; include/ymi.h states it for callers, engine/optim.py::HYPER_FIELDS fills it in this order)
enum Hyper {
    H_LR = 0, H_WD = 3,                                       // [0..2] lr of group 0..2, [3..5] weight decay of group 0..2
    H_MOMENTUM = 6, H_MAX_NORM, H_EMA_DECAY, H_EMA_TAU,       // momentum (beta1 for the Adam family), max_norm (<= 0: no clipping), EMA decay and tau
    H_NESTEROV, H_GRAD_SCALE, H_BETA2, H_EPS, H_RULE,         // nesterov (0 / 1), grad scale (1 / world), beta2 (RMSprop: alpha), eps, a Rule
    H_1M_BETA2, H_1M_BETA1,                                   // 1 - beta2, 1 - beta1: the host's double differences, as torch passes them
    H_MOMENTUM_DECAY, H_BETA1_TAIL, H_MOMENTUM_DECAY_TAIL,    // NAdam: momentum_decay, and the float32 tails of beta1 and momentum_decay
    H_COUNT
};
static_assert(H_COUNT == 20, "hyper is the 20-float array of include/ymi.h");

// state layout: float clip, float total_norm, float ema_d, float one_minus_d, int64 updates, int64 steps (optimizer steps
//               taken: Adam's t), float 1/(1-b1^t), float sqrt(1-b2^t), float c0..c3 (per-step scalars of NAdam / RAdam), double mu_product (NAdam)
struct OptState {
    float clip, norm, ema_d, ema_1md;
    long long updates;
    long long steps;
    float inv_bc1, bc2_sqrt;
    float c0, c1, c2, c3;
    double mu_product;
};
static_assert(sizeof(OptState) == 64, "OptState is the 64-byte state buffer engine/optim.py allocates");

// The workgroup's chunk: its tensor's entry, the tensor's index within the launch, and the element range [base, end).
struct Chunk {
    ymi_opt_entry e;
    int slot;
    int64_t base, end;
};
__device__ __forceinline__ Chunk opt_chunk(const ymi_opt_entry* __restrict__ tab, const int2* __restrict__ chunks, int first_tensor) {
    const int2 ch = chunks[blockIdx.x];
    Chunk c;
    c.e = tab[ch.x];
    c.slot = ch.x - first_tensor;
    c.base = (int64_t)ch.y * OPT_CHUNK;
    c.end = c.base + OPT_CHUNK < c.e.numel ? c.base + OPT_CHUNK : c.e.numel;
    return c;
}

// The one walk over a chunk.  vec (16-byte accesses allowed): thread t takes elements 4t .. 4t+3 of every 1024, four(i) on whole quads and
// one(j) on the tensor's last 1..3 elements; otherwise thread t takes element t of every 256 through one(j).
template <typename F4, typename F1>
__device__ __forceinline__ void opt_walk(int64_t base, int64_t end, bool vec, F4 four, F1 one) {
    if (vec) {
        for (int64_t i = base + threadIdx.x * 4; i < end; i += 1024) {
            if (i + 3 < end) four(i);
            else
                for (int64_t j = i; j < end; ++j) one(j);
        }
    } else {
        for (int64_t j = base + threadIdx.x; j < end; j += 256) one(j);
    }
}
__device__ __forceinline__ bool aligned16(uintptr_t bits) { return (bits & 15) == 0; }

__global__ __launch_bounds__(256) void opt_sumsq_kernel(const ymi_opt_entry* __restrict__ tab, const int2* __restrict__ chunks, int first_tensor, GradPtrs gp,
                                                        const float* __restrict__ hyper, float* __restrict__ part) {
    const Chunk c = opt_chunk(tab, chunks, first_tensor);
    const float* g = gp.g[c.slot];
    float acc = 0.f;
    if (g) {
        const float gs = hyper[H_GRAD_SCALE];
        opt_walk(
            c.base, c.end, aligned16((uintptr_t)g),
            [&](int64_t i) {
                const f32x4 v = *reinterpret_cast<const f32x4*>(g + i);
                acc += (v[0] * gs) * (v[0] * gs) + (v[1] * gs) * (v[1] * gs) + (v[2] * gs) * (v[2] * gs) + (v[3] * gs) * (v[3] * gs);
            },
            [&](int64_t j) { acc += (g[j] * gs) * (g[j] * gs); });
    }
    __shared__ float sh[4];
    acc = wave_sum(acc);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) part[blockIdx.x] = (sh[0] + sh[1]) + (sh[2] + sh[3]);
}

__global__ __launch_bounds__(256) void opt_finalize_kernel(const float* __restrict__ part, int n, const float* __restrict__ hyper, OptState* __restrict__ st) {
    __shared__ double sh[256];
    double acc = 0.0;
    for (int i = threadIdx.x; i < n; i += 256) acc += (double)part[i];
    sh[threadIdx.x] = acc;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const float norm = (float)sqrt(sh[0]);
        // torch.nn.utils.clip_grad_norm_: clip_coef = max_norm / (total_norm + 1e-6), clamped to 1
        const float coef = hyper[H_MAX_NORM] / (norm + 1e-6f);
        st->norm = norm;
        st->clip = hyper[H_MAX_NORM] > 0.f ? (coef < 1.0f ? coef : 1.0f) : 1.0f;
        const long long u = st->updates + 1;
        st->updates = u;
        // ModelEMA.decay(updates) in double, as the reference's Python float arithmetic
        const double d = (double)hyper[H_EMA_DECAY] * (1.0 - exp(-(double)u / (double)hyper[H_EMA_TAU]));
        st->ema_d = (float)d;
        st->ema_1md = (float)(1.0 - d);
        // torch.optim.Adam: bias_correction1 = 1 - beta1 ** step, bias_correction2_sqrt = (1 - beta2 ** step) ** 0.5 (Python floats)
        const long long t = st->steps + 1;
        st->steps = t;
        if (hyper[H_RULE] != 0.f) {
            // (the betas are rebuilt from their float32 COMPLEMENTS: 1 - 0.999f is off by 1.3e-5 relative, 1 - float(0.001) by 5e-8)
            const double b1 = 1.0 - (double)hyper[H_1M_BETA1], b2 = 1.0 - (double)hyper[H_1M_BETA2];
            const double bc1 = 1.0 - pow(b1, (double)t), bc2 = 1.0 - pow(b2, (double)t);
            st->inv_bc1 = (float)(1.0 / bc1);
            st->bc2_sqrt = (float)sqrt(bc2);
            const int rule = (int)hyper[H_RULE];
            if (rule == R_NADAM) {
                // torch.optim.NAdam: mu_t = beta1 * (1 - 0.5 * 0.96 ** (t * momentum_decay)), mu_product *= mu_t (Python floats)
                // beta1 and momentum_decay to double precision (float32 head + tail) - mu_product is a running product that torch rounds
                // to float32 every step, and a 1e-9 error of beta1 flips one of those roundings within ten steps
                const double b1x = (double)hyper[H_MOMENTUM] + (double)hyper[H_BETA1_TAIL];
                const double md = (double)hyper[H_MOMENTUM_DECAY] + (double)hyper[H_MOMENTUM_DECAY_TAIL];
                const double mu = b1x * (1.0 - 0.5 * pow(0.96, (double)t * md)), mu_next = b1x * (1.0 - 0.5 * pow(0.96, (double)(t + 1) * md));
                // (torch keeps mu_product as a float32 state tensor and multiplies it in place: one float32 rounding per step)
                const float mpf = (t == 1 ? 1.0f : (float)st->mu_product) * (float)mu;
                const double mp = (double)mpf;
                st->mu_product = mp;
                st->c0 = (float)((1.0 - mu) / (1.0 - mp));            // weight of grad / denom
                st->c1 = (float)(mu_next / (1.0 - mp * mu_next));     // weight of exp_avg / denom
                st->c2 = (float)bc2;                                  // denom = sqrt(exp_avg_sq / bias_correction2) + eps
            } else if (rule == R_RADAM) {
                // torch.optim.RAdam: rho_t = rho_inf - 2 t beta2^t / (1 - beta2^t); rectified step once rho_t > 5
                const double rho_inf = 2.0 / (1.0 - b2) - 1.0;
                const double rho_t = rho_inf - 2.0 * (double)t * pow(b2, (double)t) / bc2;
                if (rho_t > 5.0) {
                    st->c0 = (float)sqrt((rho_t - 4.0) * (rho_t - 2.0) * rho_inf / ((rho_inf - 4.0) * (rho_inf - 2.0) * rho_t));
                    st->c1 = 1.0f;
                } else {
                    st->c0 = 1.0f;
                    st->c1 = 0.0f;
                }
            }
        }
    }
}

// Gradient accumulation OUTSIDE autograd (reference trainer.py:305,397: nbs / batch backward passes per update): acc[i] += g[i] over the
// same entry table and chunk map; ymi_opt_entry.acc is the tensor's slice of the optimizer's accumulation arena.  A pure stream: g and
// acc read once, acc written once by the one thread that read it - no atomics, no flags, the same work on every replay of a graph.
__global__ __launch_bounds__(256) void opt_accumulate_kernel(const ymi_opt_entry* __restrict__ tab, const int2* __restrict__ chunks, int first_tensor, GradPtrs gp) {
    const Chunk c = opt_chunk(tab, chunks, first_tensor);
    const float* __restrict__ g = gp.g[c.slot];
    float* __restrict__ acc = c.e.acc;
    if (!g || !acc) return;  // no gradient this step: acc stays as it is
    opt_walk(
        c.base, c.end, aligned16((uintptr_t)g | (uintptr_t)acc),
        [&](int64_t i) {
            const f32x4 a = *reinterpret_cast<const f32x4*>(acc + i);
            const f32x4 v = *reinterpret_cast<const f32x4*>(g + i);
            *reinterpret_cast<f32x4*>(acc + i) = f32x4{a[0] + v[0], a[1] + v[1], a[2] + v[2], a[3] + v[3]};
        },
        [&](int64_t j) { acc[j] = acc[j] + g[j]; });
}

// The scalars of one update launch: what the body reads of hyper and the state record for the chunk's group.  Only the EMA pair is read
// for a chunk that is not updated (EMA-only mode, or no gradient this step).
struct StepScalars {
    float d, omd;  // EMA decay and 1 - decay
    float lr = 0.f, wd = 0.f, mom = 0.f, gscale = 0.f, b2 = 0.f, eps = 0.f, step_size = 0.f, bc2s = 1.f, omb1 = 0.f, omb2 = 0.f;
    float c0 = 0.f, c1 = 0.f, c2 = 1.f, ibc1 = 1.f, decay_mul;
    bool nest = false;
};
template <int RULE>
__device__ __forceinline__ StepScalars opt_scalars(const float* __restrict__ hyper, const OptState* __restrict__ st, int group, bool upd) {
    StepScalars k;
    k.d = st->ema_d;
    k.omd = st->ema_1md;
    if (upd) {
        k.lr = hyper[H_LR + group];
        k.wd = hyper[H_WD + group];
        k.mom = hyper[H_MOMENTUM];
        k.nest = hyper[H_NESTEROV] != 0.f;
        k.gscale = st->clip * hyper[H_GRAD_SCALE];
        if (RULE != R_SGD) {
            k.b2 = hyper[H_BETA2];
            k.eps = hyper[H_EPS];
            k.omb2 = hyper[H_1M_BETA2];
            k.omb1 = hyper[H_1M_BETA1];
            k.step_size = k.lr * st->inv_bc1;
            k.bc2s = st->bc2_sqrt;
            k.ibc1 = st->inv_bc1;
            k.c0 = st->c0; k.c1 = st->c1; k.c2 = st->c2;
        }
    }
    k.decay_mul = 1.f - k.lr * k.wd;
    return k;
}

template <typename T> struct Updated {
    T p, buf, sec, ema;
};
// One element of the update, for the vector path, its scalar tail and the scalar path.  Every multiply-add that is fused is written as fmaf and
// nothing else may be (contract(off); the Makefile builds this file with -ffp-contract=fast-honor-pragmas): left to the compiler, the packed-math
// pass fused the EMA's multiply-add in some lanes of a float4 and not in others, so the same element rounded differently by its position
// and by the alignment of its tensor.  tests/test_gpu_optim_exact.py holds the paths to bit equality.  Which sums are fused and which are
// not is what the vector path of parameters and moments had been compiled to all along: aligned tensors step as they always did.
template <int RULE>
__device__ __forceinline__ Updated<float> opt_update(const StepScalars& k, bool upd, float pv, float gv, float bv, float sv, float ev) {
#pragma clang fp contract(off)
    Updated<float> o = {pv, bv, sv, 0.f};
    const auto scaled_grad = [&]() { return k.wd != 0.f ? gv * k.gscale + k.wd * pv : gv * k.gscale; };  // grad * clip / world, then grad.add(param, alpha=weight_decay)
    const auto first_moment = [&](float diff) { return fmaf(diff, k.omb1, bv); };         // exp_avg.lerp_(grad, 1 - beta1), diff = grad - exp_avg
    const auto second_moment = [&](float gr) { return fmaf(k.omb2 * gr, gr, sv * k.b2); };  // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value=1 - beta2)
    if (upd) {
        constexpr bool lerps = RULE >= R_ADAMW && RULE <= R_RADAM, squares = RULE != R_SGD && RULE != R_ADAMAX;
        // AdamW decays the parameter, not the gradient: nothing between the scaling and the difference, and its lerp takes both in one fma
        float gr = RULE == R_ADAMW ? gv * k.gscale : scaled_grad();
        if (lerps) o.buf = first_moment(RULE == R_ADAMW ? fmaf(gv, k.gscale, -bv) : gr - bv);
        if (squares) o.sec = second_moment(gr);
        if constexpr (RULE == R_SGD) {
            o.buf = fmaf(bv, k.mom, gr);                      // buf.mul_(momentum).add_(grad)   (first step: buf = 0 -> grad)
            gr = k.nest ? fmaf(k.mom, o.buf, gr) : o.buf;     // grad.add(buf, alpha=momentum)
            o.p = fmaf(-k.lr, gr, pv);                        // param.add_(grad, alpha=-lr)
        } else if constexpr (RULE == R_ADAMW || RULE == R_ADAM) {
            const float denom = sqrtf(o.sec) / k.bc2s + k.eps;  // (exp_avg_sq.sqrt() / bias_correction2_sqrt).add_(eps)
            // param.addcdiv_(exp_avg, denom, value=-lr / bias_correction1); AdamW: param.mul_(1 - lr * weight_decay) first, two products and a difference
            o.p = RULE == R_ADAMW ? pv * k.decay_mul - k.step_size * (o.buf / denom) : fmaf(-k.step_size, o.buf / denom, pv);
        } else if constexpr (RULE == R_ADAMAX) {
            o.sec = fmaxf(sv * k.b2, fabsf(gr) + k.eps);      // exp_inf = max(exp_inf * beta2, |grad| + eps)
            o.p = fmaf(-k.step_size, o.buf / o.sec, pv);      // param.addcdiv_(exp_avg, exp_inf, value=-lr / bias_correction1)
        } else if constexpr (RULE == R_NADAM) {
            const float denom = sqrtf(o.sec / k.c2) + k.eps;        // exp_avg_sq.div(bias_correction2).sqrt().add_(eps)
            const float p1 = pv - (k.lr * k.c0) * (gr / denom);     // param.addcdiv_(grad, denom, value=-lr (1 - mu) / (1 - mu_product))
            o.p = p1 - (k.lr * k.c1) * (o.buf / denom);             // param.addcdiv_(exp_avg, denom, value=-lr mu_next / (1 - mu_product mu_next))
        } else if constexpr (RULE == R_RADAM) {
            const float bce = o.buf * k.ibc1;                       // exp_avg / bias_correction1
            if (k.c1 != 0.f) o.p = pv - ((bce * k.lr) * (k.bc2s / (sqrtf(o.sec) + k.eps))) * k.c0;  // bias_corrected_exp_avg * lr * adaptive * rect
            else o.p = pv - bce * k.lr;
        } else {                                                    // torch.optim.RMSprop(momentum > 0), alpha = b2
            o.buf = fmaf(bv, k.mom, gr / (sqrtf(o.sec) + k.eps));   // buf.mul_(momentum).addcdiv_(grad, avg), avg = square_avg.sqrt() + eps
            o.p = fmaf(-k.lr, o.buf, pv);
        }
    }
    o.ema = fmaf(ev, k.d, k.omd * o.p);                            // v *= d; v += (1 - d) * model value
    return o;
}

// ... and the same body on each of four
template <int RULE>
__device__ __forceinline__ Updated<f32x4> opt_update(const StepScalars& k, bool upd, f32x4 pv, f32x4 gv, f32x4 bv, f32x4 sv, f32x4 ev) {
    Updated<float> e[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) e[r] = opt_update<RULE>(k, upd, pv[r], gv[r], bv[r], sv[r], ev[r]);
    return {{e[0].p, e[1].p, e[2].p, e[3].p}, {e[0].buf, e[1].buf, e[2].buf, e[3].buf}, {e[0].sec, e[1].sec, e[2].sec, e[3].sec}, {e[0].ema, e[1].ema, e[2].ema, e[3].ema}};
}

// T = float: one element; T = f32x4: four, in one 16-byte access per operand
template <typename T> __device__ __forceinline__ T opt_load(const float* q, int64_t i, bool on) { return on ? *reinterpret_cast<const T*>(q + i) : T{}; }
template <typename T> __device__ __forceinline__ void opt_store(float* q, int64_t i, bool on, T v) {
    if (on) *reinterpret_cast<T*>(q + i) = v;
}

// MODE 0: parameters with gradients (update + EMA);  MODE 1: EMA only (buffers, frozen parameters)
// RULE: a compile-time parameter, one straight-line body per rule
template <int MODE, int RULE>
__global__ __launch_bounds__(256) void opt_update_kernel(const ymi_opt_entry* __restrict__ tab, const int2* __restrict__ chunks, int first_tensor, GradPtrs gp,
                                                         const float* __restrict__ hyper, const OptState* __restrict__ st) {
    const Chunk c = opt_chunk(tab, chunks, first_tensor);
    const float* g = MODE == 0 ? gp.g[c.slot] : nullptr;
    float* p = c.e.param;
    float* buf = c.e.momentum;
    float* sec = c.e.second;  // Adam: exp_avg_sq
    float* ema = c.e.ema;
    const bool upd = MODE == 0 && g;
    constexpr bool two_moments = RULE != R_SGD;  // every rule but SGD keeps a second per-element state (RMSprop: square_avg)
    const StepScalars k = opt_scalars<RULE>(hyper, st, c.e.group, upd);
    // load what this mode and rule reads, run the body, store what it writes
    const auto elem = [&](int64_t i, auto zero) {
        using T = decltype(zero);
        const T pv = opt_load<T>(p, i, true), gv = opt_load<T>(g, i, upd), bv = opt_load<T>(buf, i, upd && buf), sv = opt_load<T>(sec, i, upd && two_moments),
                ev = opt_load<T>(ema, i, ema != nullptr);
        const Updated<T> o = opt_update<RULE>(k, upd, pv, gv, bv, sv, ev);
        opt_store<T>(p, i, upd, o.p);
        opt_store<T>(buf, i, upd && buf, o.buf);
        opt_store<T>(sec, i, upd && two_moments, o.sec);
        opt_store<T>(ema, i, ema != nullptr, o.ema);
    };
    opt_walk(
        c.base, c.end, aligned16((uintptr_t)p | (uintptr_t)g | (uintptr_t)buf | (uintptr_t)sec | (uintptr_t)ema), [&](int64_t i) { elem(i, f32x4{}); },
        [&](int64_t j) { elem(j, 0.f); });
}

// what every entry point asks of a launch range; `rest`: the entry point's other pointers that must not be null
int opt_check(const ymi_opt_entry* table, const int32_t* chunk_map, int32_t first_tensor, int32_t n_tensors, int64_t n_chunks, bool rest, const char* what) {
    YMI_CHECK_ARG(table && chunk_map && rest, "%s: null argument", what);
    YMI_CHECK_ARG(first_tensor >= 0 && n_tensors >= 1 && n_tensors <= OPT_GRADS, "%s: 1..%d tensors per launch", what, OPT_GRADS);
    YMI_CHECK_ARG(n_chunks >= 1 && n_chunks < (1ll << 31), "%s: chunk count", what);
    return YMI_OK;
}

GradPtrs grad_ptrs(const float* const* host_grads, int n_tensors) {
    GradPtrs gp{};
    for (int i = 0; host_grads && i < n_tensors; ++i) gp.g[i] = host_grads[i];
    return gp;
}
}  // namespace

extern "C" int64_t ymi_opt_chunk_elems(void) { return OPT_CHUNK; }

extern "C" int ymi_opt_grad_norm(const ymi_opt_entry* table, const int32_t* chunk_map, int32_t first_tensor, int32_t n_tensors, int64_t n_chunks,
                                 const float* const* host_grads, const float* hyper, float* partials, int64_t partials_offset, int64_t partials_total,
                                 void* state, int32_t finalize, void* stream) {
    int rc = opt_check(table, chunk_map, first_tensor, n_tensors, n_chunks, hyper && state, "opt_grad_norm");
    if (rc) return rc;
    YMI_CHECK_ARG(host_grads && partials && partials_offset >= 0 && partials_offset + n_chunks <= partials_total, "opt_grad_norm: partials range");
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(opt_sumsq_kernel, dim3((unsigned)n_chunks), dim3(256), 0, s, table, reinterpret_cast<const int2*>(chunk_map), first_tensor,
                       grad_ptrs(host_grads, n_tensors), hyper, partials + partials_offset);
    if (finalize) hipLaunchKernelGGL(opt_finalize_kernel, dim3(1), dim3(256), 0, s, partials, (int)partials_total, hyper, reinterpret_cast<OptState*>(state));
    YMI_CHECK_LAUNCH("opt_grad_norm");
    return YMI_OK;
}

extern "C" int ymi_opt_update(const ymi_opt_entry* table, const int32_t* chunk_map, int32_t first_tensor, int32_t n_tensors, int64_t n_chunks,
                              const float* const* host_grads, const float* hyper, const void* state, int32_t rule, void* stream) {
    int rc = opt_check(table, chunk_map, first_tensor, n_tensors, n_chunks, hyper && state, "opt_update");
    if (rc) return rc;
    YMI_CHECK_ARG(rule >= 0 && rule < R_COUNT, "opt_update: rule 0 (SGD), 1 (AdamW), 2 (Adam), 3 (Adamax), 4 (NAdam), 5 (RAdam) or 6 (RMSprop)");
    // the kernel of each Rule, and the EMA-only pass
    static const decltype(&opt_update_kernel<0, R_SGD>) kernels[R_COUNT + 1] = {opt_update_kernel<0, R_SGD>, opt_update_kernel<0, R_ADAMW>, opt_update_kernel<0, R_ADAM>,    opt_update_kernel<0, R_ADAMAX>,
                                                     opt_update_kernel<0, R_NADAM>, opt_update_kernel<0, R_RADAM>, opt_update_kernel<0, R_RMSPROP>, opt_update_kernel<1, R_SGD>};
    hipLaunchKernelGGL(kernels[host_grads ? rule : R_COUNT], dim3((unsigned)n_chunks), dim3(256), 0, (hipStream_t)stream, table, reinterpret_cast<const int2*>(chunk_map),
                       first_tensor, grad_ptrs(host_grads, n_tensors), hyper, reinterpret_cast<const OptState*>(state));
    YMI_CHECK_LAUNCH("opt_update");
    return YMI_OK;
}

extern "C" int ymi_opt_grad_accumulate(const ymi_opt_entry* table, const int32_t* chunk_map, int32_t first_tensor, int32_t n_tensors, int64_t n_chunks,
                                       const float* const* host_grads, void* stream) {
    int rc = opt_check(table, chunk_map, first_tensor, n_tensors, n_chunks, host_grads != nullptr, "opt_grad_accumulate");
    if (rc) return rc;
    hipLaunchKernelGGL(opt_accumulate_kernel, dim3((unsigned)n_chunks), dim3(256), 0, (hipStream_t)stream, table, reinterpret_cast<const int2*>(chunk_map), first_tensor,
                       grad_ptrs(host_grads, n_tensors));
    YMI_CHECK_LAUNCH("opt_grad_accumulate");
    return YMI_OK;
}
