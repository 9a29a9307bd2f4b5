/* brainevent_amd.h — C ABI of libbrainevent_amd.so (MI355X / gfx950 spike-triggered SpMV/SpMM engine).
 *
 * This is the drop-in boundary for the ONE hot path of chaobrain/brainevent that this repository
 * accelerates: BinaryArray @ {CSR, CSC, dense, JITC{Scalar,Normal,Uniform}{R,C}, FixedNumConn}.
 *
 * What it replaces in the reference (paths relative to the reference checkout, read as text only):
 *   the `// @BE <name>` native entry points that brainevent/_op/kernix_codegen.py:617-736 wraps into
 *   `extern "C" XLA_FFI_Error* be_<name>(XLA_FFI_CallFrame*)` and that the Python side reaches through
 *   `jax.ffi.ffi_call("<module>.<name>", …)`.  Here the same per-variant naming grammar is kept
 *   (`<op>_<homo|hetero>_<f32|f64|f16|bf16>_<bool|float>`), but the calling convention is a plain C one:
 *   raw device pointers + sizes + an explicit hipStream_t, `int` status return, no XLA/JAX types,
 *   no torch types.  Each declaration cites the reference interface it stands in for.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless the parameter name ends in `_host`;
 *   - the caller owns every buffer (the library allocates nothing that outlives a call);
 *   - `stream` is a hipStream_t passed as void* (NULL = the default stream); calls are asynchronous
 *     on that stream unless stated otherwise;
 *   - return value 0 = success, negative = error (see BE_ERR_*); `be_last_error()` returns a
 *     thread-local message.  The library never aborts the process;
 *   - bool spikes are any 1-byte integer buffer, active when != 0; float spikes are f32, active when > 0
 *     (reference: brainevent/include/cuda_common.h:120-131);
 *   - indices are int32; indptr is int32 or int64 (`indptr_is_i64`)
 *     (reference: brainevent/include/brainevent/dispatch.h:184-215).
 */
#ifndef BRAINEVENT_AMD_H
#define BRAINEVENT_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BE_OK 0
#define BE_ERR_INVALID (-1)
#define BE_ERR_WORKSPACE (-2)
#define BE_ERR_HIP (-3)
#define BE_ERR_RANGE (-4)
#define BE_ERR_UNSUPPORTED (-5)

/* weight / output dtype codes and spike dtype codes used by the generic entry points */
#define BE_F32 0
#define BE_F64 1
#define BE_F16 2
#define BE_BF16 3
#define BE_SPIKE_BOOL 0
#define BE_SPIKE_FLOAT 1
/* bit-packed events: uint32 words, bit i%32 of word i/32 (rows of ceil(n/32) words in a batch); the layout of the
 * reference's `bitpack` (brainevent/_event/bitpack_binary.py:32-75).  Accepted by be_compact_spikes* and by the
 * scatter entry points that start with a compaction (be_binary_csrmv/mm_t, *_t_plan, *_t_binned). */
#define BE_SPIKE_BITS 2
/* already-compacted events (single vector, scatter entry points only): `spikes` is a HOST pointer to a be_spike_ids_t
 * whose two fields are DEVICE pointers — the first *n_active entries of active_ids are the active positions, each
 * < m and listed once (caller contract; what be_compact_spikes produces).  The call skips its compaction kernel. */
#define BE_SPIKE_IDS 3
typedef struct be_spike_ids {
  const uint32_t* active_ids;
  const uint32_t* n_active;
} be_spike_ids_t;

typedef void* be_stream_t; /* hipStream_t */

/* ------------------------------------------------------------------------------------------------
 * library / runtime
 * ---------------------------------------------------------------------------------------------- */
int be_version(void);                 /* 10000*major + 100*minor + patch */
const char* be_last_error(void);      /* thread-local, valid until the next failing call on this thread */
int be_device_count(void);            /* number of visible HIP devices, or a negative BE_ERR_* */
int64_t be_device_max_grid_y(void);   /* hipDeviceProp_t::maxGridSize[1] of the current device (the JIT products refuse a shape
                                         whose walk takes more chunks than this), or a negative BE_ERR_* */
const char* be_build_arch(void);      /* "gfx950" */
/* HIP-event timing of each op's dominant kernel, recorded on the op's own stream.
 * enable(n) arms n record slots (0 disarms); read() synchronises and returns the number of
 * records copied to ms_host (kernel durations in milliseconds, in call order) and rearms. */
int be_profile_enable(int max_records);
int be_profile_read(float* ms_host, int capacity);
/* Diagnostic: the read-only streaming rate of this device in the caller's own run (the ceiling a read-dominated kernel is held
 * against): `repeats` passes of 16-byte-per-lane loads over buf[0 .. bytes) (16-byte aligned, device memory) between
 * two HIP events on `stream`; synchronises; *ms_per_pass = average pass time.  sink4: 4 writable device bytes. */
int be_diag_stream_read(const void* buf, int64_t bytes, int repeats, void* sink4, float* ms_per_pass, be_stream_t stream);
/* releases the little the library keeps between calls (profiling events); exchange handles have be_exchange_destroy */
int be_shutdown(void);

/* ----------------------------------------------------------------------------------------------
 * Neuron half of the COBA step loop (the reference example composes the same dynamics from brainstate
 * modules, examples/COBA_2005.py:35-87): ONE fused update of n conductance-based LIF neurons with exponential synapses,
 * in place.  Per neuron, every operation rounded separately in this order (so it reproduces the plain elementwise
 * formulation bit for bit):
 *   g_exc = g_exc * decay_exc + in_exc;   g_inh = g_inh * decay_inh + in_inh          (in_*: this step's scatter outputs)
 *   i_syn = (g_exc * (e_exc - v) + g_inh * (e_inh - v)) * syn_scale
 *   dv    = (-(v - v_rest) + i_syn + i_ext) * (dt / tau_m)
 *   active = refractory <= 0;  v' = active ? v + dv : v;  spike = active && v' >= v_th
 *   v = spike ? v_reset : v';  refractory = spike ? t_ref : refractory - dt;  spikes_out = spike (1 byte);
 *   spike_count += spike (optional, may be NULL)
 * A time step of the network is then: scatter(spikes_exc) -> in_exc, scatter(spikes_inh) -> in_inh, be_lif_coba_step.
 * ---------------------------------------------------------------------------------------------- */
int be_lif_coba_step(float* v, float* g_exc, float* g_inh, float* refractory, const float* in_exc, const float* in_inh,
                     uint8_t* spikes_out, float* spike_count, int64_t n, double dt, double tau_m, double v_rest, double v_th,
                     double v_reset, double t_ref, double e_exc, double e_inh, double decay_exc, double decay_inh, double i_ext,
                     double syn_scale, be_stream_t stream);
/* The same step; the spikes are ALSO (or only: spikes_out may then be NULL) written bit-packed, spike_bits_out[ceil(n / 32)]
 * (bit i % 32 of word i / 32; bits past n are 0) — the form every scatter entry point takes as BE_SPIKE_BITS and
 * be_exchange_allgather_bits / be_exchange_post gather from where it lies: a step loop that keeps its spikes as words has no
 * pack launch anywhere (the reference packs per call, brainevent/_jit_scalar/binary_jitsmv.cu:107-125). */
int be_lif_coba_step_packed(float* v, float* g_exc, float* g_inh, float* refractory, const float* in_exc, const float* in_inh,
                            uint8_t* spikes_out, uint32_t* spike_bits_out, float* spike_count, int64_t n, double dt, double tau_m,
                            double v_rest, double v_th, double v_reset, double t_ref, double e_exc, double e_inh,
                            double decay_exc, double decay_inh, double i_ext, double syn_scale, be_stream_t stream);
/* The CURRENT-based twin (reference example examples/CUBA_2005.py:35-66: LIF V_rest -49 mV, V_th -50 mV, V_reset -60 mV, tau 20 ms,
 * refractory 5 ms; Expon synapses tau 5 / 10 ms with CUBA outputs, weights 1.62 / -9.0 mS): the same update with
 *   i_syn = (g_exc + g_inh) * syn_scale
 * in place of the conductance term (no reversal potentials; an inhibitory projection carries a negative weight).  Every other line,
 * the rounding order and the spike outputs are those of be_lif_coba_step / be_lif_coba_step_packed. */
int be_lif_cuba_step(float* v, float* g_exc, float* g_inh, float* refractory, const float* in_exc, const float* in_inh,
                     uint8_t* spikes_out, float* spike_count, int64_t n, double dt, double tau_m, double v_rest, double v_th,
                     double v_reset, double t_ref, double decay_exc, double decay_inh, double i_ext, double syn_scale,
                     be_stream_t stream);
int be_lif_cuba_step_packed(float* v, float* g_exc, float* g_inh, float* refractory, const float* in_exc, const float* in_inh,
                            uint8_t* spikes_out, uint32_t* spike_bits_out, float* spike_count, int64_t n, double dt, double tau_m,
                            double v_rest, double v_th, double v_reset, double t_ref, double decay_exc, double decay_inh, double i_ext,
                            double syn_scale, be_stream_t stream);
/* Either step (current_based = 0: be_lif_coba_step_packed, 1: be_lif_cuba_step_packed; e_exc / e_inh ignored then) with the two
 * inputs multiplied by in_scale_exc / in_scale_inh first (g = g * decay + in * in_scale, each operation rounded separately).  What it
 * is for: ONE scatter for both projections of a network — the excitatory and the inhibitory matrix stacked into one n x 2n matrix
 * with weight 1 (columns [0, n) = targets of the excitatory rows, [n, 2n) = targets of the inhibitory rows): its output halves are
 * the synaptic COUNTS, the weights are applied here — count * w is rounded exactly as it is inside a scatter with weight w, so the
 * step equals the two-projection formulation bit for bit with half the launches (examples/coba_2005.py `combined=True`).
 * in_scale = 1.0 reproduces the plain entry points. */
int be_lif_step_scaled_packed(int current_based, float* v, float* g_exc, float* g_inh, float* refractory, const float* in_exc,
                              const float* in_inh, double in_scale_exc, double in_scale_inh, uint8_t* spikes_out,
                              uint32_t* spike_bits_out, float* spike_count, int64_t n, double dt, double tau_m, double v_rest,
                              double v_th, double v_reset, double t_ref, double e_exc, double e_inh, double decay_exc,
                              double decay_inh, double i_ext, double syn_scale, be_stream_t stream);

/* ----------------------------------------------------------------------------------------------
 * The differentiable neuron between two products (brainevent_amd/csrc/be_neuron_sg.hip; no native counterpart in the reference,
 * which leaves the neuron to brainstate): a leaky integrate-and-fire neuron without synapse state or refractory period, T time
 * steps of N independent slots (a batch is more slots) in ONE launch, and its backward pass with a surrogate gradient in one
 * more.  All arrays f32; x, s_out, v_seq, h_save, g_s, g_vseq, g_x are [T, N] row-major, v0, v_last, g_vlast, g_v0 are [N].
 * beta, v_th, v_reset, alpha are rounded to f32 once on the host; per slot i every operation is rounded separately, in this
 * order (so both passes reproduce the plain elementwise f32 formulation bit for bit; there is no transcendental):
 *   forward, t = 0 .. T-1, v = v0[i] (v0 NULL: 0):
 *     h = (beta * v) + x[t][i];   s = h >= v_th   (a NaN does not spike)
 *     v = BE_LIF_RESET_HARD: s ? v_reset : h      BE_LIF_RESET_SOFT: s ? h - v_th : h
 *     s_out[t][i] = s ? 1 : 0;   v_seq[t][i] = v  (v_seq may be NULL);   h_save[t][i] = h  (h_save may be NULL: no backward pass)
 *   then v_last[i] = v.
 *   backward, t = T-1 .. 0, carry = g_vlast[i] (NULL: 0), h = h_save[t][i], u = h - v_th, s = h >= v_th:
 *     g_vo = carry + g_vseq[t][i]                 (the addition only if g_vseq is given)
 *     sg   = BE_LIF_SG_FAST_SIGMOID: d = 1 + alpha * |u|;  sg = 1 / (d * d)
 *            BE_LIF_SG_ATAN:         q = f32(pi / 2 * alpha) * u;  sg = f32(alpha / 2) / (1 + q * q)
 *            BE_LIF_SG_TRIANGLE:     a = 1 - alpha * |u|;  sg = alpha * (a > 0 ? a : 0)
 *     g_sp = g_s[t][i] (g_s NULL: 0);  unless detach_reset:  hard: g_sp = g_sp + g_vo * (v_reset - h)   soft: g_sp = g_sp - g_vo * v_th
 *     g_h  = g_sp * sg + (hard ? (s ? 0 : g_vo) : g_vo);   g_x[t][i] = g_h;   carry = beta * g_h
 *   then g_v0[i] = carry (g_v0 may be NULL).
 * T == 0 or N == 0: BE_OK, nothing launched.  BE_ERR_INVALID: x, s_out, v_last / h_save, g_x NULL; T < 0 or N < 0; an unknown
 * reset_mode or surrogate; alpha <= 0.  A lane owns 4 consecutive slots and moves them with 16-byte accesses when N % 4 == 0 and
 * every given pointer is 16-byte aligned, one slot with 4-byte accesses otherwise; the results do not depend on which.
 * ---------------------------------------------------------------------------------------------- */
#define BE_LIF_RESET_HARD 0
#define BE_LIF_RESET_SOFT 1
#define BE_LIF_SG_FAST_SIGMOID 0
#define BE_LIF_SG_ATAN 1
#define BE_LIF_SG_TRIANGLE 2
int be_lif_sg_forward(const float* x, const float* v0, float* s_out, float* v_seq, float* h_save, float* v_last, int64_t T,
                      int64_t N, double beta, double v_th, double v_reset, int reset_mode, be_stream_t stream);
int be_lif_sg_backward(const float* h_save, const float* g_s, const float* g_vseq, const float* g_vlast, float* g_x, float* g_v0,
                       int64_t T, int64_t N, double beta, double v_th, double v_reset, int reset_mode, int surrogate, double alpha,
                       int detach_reset, be_stream_t stream);
/* The same neuron with beta and v_th read from DEVICE memory (brainevent_amd/csrc/be_neuron_sg.hip; the reduce:
 * be_neuron_sg_reduce.hip): each is an f32 array with a period P >= 1 that divides N, and slot i of a step uses beta[i % beta_period], v_th[i % vth_period] (P = 1: one shared
 * value; P = N / R: one value per neuron under R leading batch rows).  No value crosses to the host: a parameter updated in place
 * is seen by the next call and by the next replay of a captured graph.  v_reset and alpha stay host scalars.
 *   forward: the forward pass above with beta_i, th_i in place of the two constants — the same operations, order and roundings.
 *   backward: the backward pass above with beta_i, th_i, and per slot two f32 accumulators a_b = a_th = +0; at step t, once
 *   g_vo, sg, g_sp, g_h are formed:
 *     v_prev = t > 0 ? reset(h_save[t-1][i]) : v0[i] (v0 NULL: 0)
 *              reset(h') = hard: (h' >= th_i ? v_reset : h')   soft: (h' >= th_i ? h' - th_i : h')
 *     a_b  = a_b + (g_h * v_prev)                                              (only if g_beta_slot is given)
 *     d    = g_sp * sg  (the product that enters g_h);  soft only: d = d + (s ? g_vo : 0);  a_th = a_th - d
 *                                                                              (only if g_vth_slot is given)
 *   then g_beta_slot[i] = a_b, g_vth_slot[i] = a_th ([N] each).  The soft reset's direct term is there with and without
 *   detach_reset (the derivative of h - s * v_th in v_th at fixed s).  g_v0, g_beta_slot, g_vth_slot may be NULL, and a NULL
 *   output costs neither its arithmetic nor its store; v0 is read only when g_beta_slot is given.  Every operation is rounded
 *   separately, so all outputs equal the elementwise f32 formulation bit for bit; a NaN stays in its slot.
 * be_lif_sg_reduce_slots: out[p] = sum over r < N / P of slot[r * P + p], p < P — accumulated in f64 in an order the shape alone
 *   fixes, rounded to f32 once, no atomics (two calls give identical bits):
 *     |f64(out[p]) - exact| <= 2^-24 |exact| + (N / P) 2^-52 sum |slot| + 2^-149.
 *   workspace: be_lif_sg_reduce_slots_workspace_bytes(N, P) bytes, 8-byte aligned, caller-owned (0 bytes unless P == 1: NULL then).
 * BE_ERR_INVALID, beyond the codes above: a period < 1 or not dividing N; beta or v_th NULL; slot or out NULL; a workspace that is
 * NULL or too small where one is needed.  The 16-byte kernels also need each period to be 1 or a multiple of 4 with a 16-byte
 * aligned base; the results do not depend on which kernel runs. */
int be_lif_sg_forward_params(const float* x, const float* v0, const float* beta, int64_t beta_period, const float* v_th,
                             int64_t vth_period, float* s_out, float* v_seq, float* h_save, float* v_last, int64_t T, int64_t N,
                             double v_reset, int reset_mode, be_stream_t stream);
int be_lif_sg_backward_params(const float* h_save, const float* v0, const float* g_s, const float* g_vseq, const float* g_vlast,
                              const float* beta, int64_t beta_period, const float* v_th, int64_t vth_period, float* g_x, float* g_v0,
                              float* g_beta_slot, float* g_vth_slot, int64_t T, int64_t N, double v_reset, int reset_mode,
                              int surrogate, double alpha, int detach_reset, be_stream_t stream);
int64_t be_lif_sg_reduce_slots_workspace_bytes(int64_t N, int64_t P);
int be_lif_sg_reduce_slots(const float* slot, int64_t N, int64_t P, float* out, void* workspace, int64_t workspace_bytes,
                           be_stream_t stream);
/* The differentiable neuron with a synaptic current and an optional adaptive threshold (brainevent_amd/csrc/be_neuron_sg.hip):
 * per slot a current c, a membrane v and, if adaptive, a trace a of the slot's own spikes that raises its threshold (ALIF / LSNN).
 * T steps of N slots in ONE launch forwards and one backwards, as above.  Everything is f32; x, s_out, v_seq, h_save, th_save, g_s,
 * g_vseq, g_x are [T, N] row-major, the others [N].  syn_decay, beta, v_th, v_reset, rho, kappa, alpha are doubles rounded to f32
 * once on the host.  No FMA contraction (#pragma clang fp contract(off)): per slot i every operation is its own rounding, in
 * exactly this order.
 *   forward, t = 0 .. T-1, c = c0[i], v = v0[i], a = a0[i] (a NULL pointer means 0):
 *     c  = (syn_decay * c) + x[t][i]
 *     h  = (beta * v) + c
 *     th = adaptive ? v_th + (kappa * a) : v_th
 *     s  = h >= th                                          (a NaN does not spike)
 *     v  = hard: s ? v_reset : h        soft: s ? h - v_th : h     (soft subtracts the BASE threshold, as Bellec et al. 2018)
 *     a  = adaptive ? (rho * a) + (s ? 1 : 0) : unused
 *     s_out[t][i] = s ? 1 : 0;  v_seq[t][i] = v (if given);  h_save[t][i] = h (if given);  th_save[t][i] = th (adaptive and h_save given)
 *   after the loop  c_last[i] = c;  v_last[i] = v;  a_last[i] = a (adaptive)
 *   backward, t = T-1 .. 0, carries cc = g_clast[i], cv = g_vlast[i], ca = g_alast[i] (NULL means 0).  Per step h = h_save[t][i],
 *   th = adaptive ? th_save[t][i] : v_th, s = h >= th, u = h - th:
 *     g_vo = cv + g_vseq[t][i]                              (the addition only if g_vseq is given)
 *     sg   = the surrogate above at u (BE_LIF_SG_FAST_SIGMOID / _ATAN / _TRIANGLE: the same operations and constants)
 *     g_sp = g_s[t][i] (NULL: 0);   adaptive: g_sp = g_sp + ca
 *            unless detach_reset:   hard: g_sp = g_sp + g_vo * (v_reset - h)     soft: g_sp = g_sp - g_vo * v_th
 *     g_u  = g_sp * sg
 *     g_h  = g_u + (hard ? (s ? 0 : g_vo) : g_vo)
 *     g_c  = cc + g_h;    g_x[t][i] = g_c
 *     cc   = syn_decay * g_c;    cv = beta * g_h;    adaptive: ca = (rho * ca) - (kappa * g_u)
 *   after the loop  g_c0[i] = cc;  g_v0[i] = cv;  g_a0[i] = ca   (each may be NULL)
 * detach_reset cuts only the reset's path through the spike; the adaptation's path (+ ca) is always there.  With syn_decay = 0,
 * adaptive = 0 and c0, g_clast zero the two passes are be_lif_sg_forward / be_lif_sg_backward (up to the sign of a zero sum).
 * T == 0 or N == 0: BE_OK, nothing launched.  BE_ERR_INVALID: x, s_out, c_last, v_last / h_save, g_x NULL; adaptive with a_last
 * NULL, with h_save given and th_save NULL (forward), with th_save NULL (backward); T < 0 or N < 0; an unknown reset_mode or
 * surrogate; alpha <= 0.  With adaptive == 0 the five adaptation pointers (a0, th_save, a_last / th_save, g_alast, g_a0) are neither
 * read nor written.  16-byte accesses when N % 4 == 0 and every given pointer is 16-byte aligned, 4-byte accesses otherwise; the
 * results do not depend on which. */
int be_lif_syn_sg_forward(const float* x, const float* c0, const float* v0, const float* a0, float* s_out, float* v_seq,
                          float* h_save, float* th_save, float* c_last, float* v_last, float* a_last, int64_t T, int64_t N,
                          double syn_decay, double beta, double v_th, double v_reset, double rho, double kappa, int reset_mode,
                          int adaptive, be_stream_t stream);
int be_lif_syn_sg_backward(const float* h_save, const float* th_save, const float* g_s, const float* g_vseq, const float* g_clast,
                           const float* g_vlast, const float* g_alast, float* g_x, float* g_c0, float* g_v0, float* g_a0, int64_t T,
                           int64_t N, double syn_decay, double beta, double v_th, double v_reset, double rho, double kappa,
                           int reset_mode, int surrogate, double alpha, int adaptive, int detach_reset, be_stream_t stream);
/* The same neuron with syn_decay, beta, v_th, rho and kappa read from DEVICE memory (brainevent_amd/csrc/be_neuron_sg.hip; the reduce
 * is be_lif_sg_reduce_slots above, called once per parameter that needs a gradient).  Each of the five is an f32 array with a period
 * P >= 1 of its own that divides N; slot i of a step uses param[i % P] — write sd_i, beta_i, vth_i, rho_i, kappa_i.  v_reset and
 * alpha stay host scalars.  Every operation is rounded on its own, in this order and with these parentheses.
 *   forward, t = 0 .. T-1, c = c0[i], v = v0[i], a = a0[i] (a NULL pointer means 0):
 *     a_in = a                                                        (adaptive)
 *     c  = (sd_i * c) + x[t][i]
 *     h  = (beta_i * v) + c
 *     th = adaptive ? vth_i + (kappa_i * a_in) : vth_i
 *     s  = h >= th
 *     v  = hard: s ? v_reset : h        soft: s ? h - vth_i : h       (the BASE threshold, as above)
 *     a  = adaptive ? (rho_i * a_in) + (s ? 1 : 0)
 *     s_out, v_seq, h_save as above;   c_save[t][i] = c (if given);   a_save[t][i] = a_in (adaptive and h_save given)
 *   after the loop c_last, v_last, a_last
 *   a_save takes the place of th_save: the backward pass forms th = vth_i + (kappa_i * a_save[t][i]) with the same two operations,
 *   so it has the same bits.  c_save is needed for g_sd_slot alone and may be NULL otherwise.
 *   backward, t = T-1 .. 0: the step above verbatim with the slot's own five values and the recomputed th, and up to five f32
 *   accumulators per slot, each +0 at the start and each kept only if its output pointer is given.  With a_in = a_save[t][i], ca_in
 *   the trace's carry BEFORE this step updates it, and g_c = g_x[t][i]:
 *     th_prev = adaptive ? vth_i + (kappa_i * a_save[t-1][i]) : vth_i
 *     v_prev  = t > 0 ? membrane_after(h_save[t-1][i], th_prev, vth_i, v_reset) : v0[i]   (NULL: 0)
 *               membrane_after(h', th', vth, v_reset) = hard: (h' >= th' ? v_reset : h')   soft: (h' >= th' ? h' - vth : h')
 *     c_prev  = t > 0 ? c_save[t-1][i] : c0[i]                                            (NULL: 0)
 *     acc_sd    = acc_sd    + (g_c * c_prev)
 *     acc_beta  = acc_beta  + (g_h * v_prev)
 *     d = g_u;  soft only: d = d + (s ? g_vo : 0);      acc_vth = acc_vth - d             (with and without detach_reset)
 *     acc_kappa = acc_kappa - (g_u * a_in)                                                (adaptive)
 *     acc_rho   = acc_rho   + (ca_in * a_in)                                              (adaptive)
 *   after the loop: g_sd_slot[i], g_beta_slot[i], g_vth_slot[i], g_rho_slot[i], g_kappa_slot[i]   ([N] each; each may be NULL)
 *   v_prev is decided with the ADAPTIVE threshold of step t - 1; acc_rho uses the carry that ARRIVES at step t.  c0 is read only
 *   when g_sd_slot is given, v0 only when g_beta_slot is.
 * T == 0 or N == 0: BE_OK, nothing launched.  BE_ERR_INVALID: everything be_lif_syn_sg_forward / _backward refuse (a_save in
 * th_save's place); a period < 1 or not dividing N; syn_decay, beta or v_th NULL; adaptive with rho or kappa NULL; c_save NULL
 * while g_sd_slot is given.  With adaptive == 0 the adaptation's pointers and periods (a0, rho, kappa, a_save, a_last / a_save,
 * g_alast, g_a0, g_rho_slot, g_kappa_slot) are neither read nor written.  16-byte accesses when N % 4 == 0, every given pointer is
 * 16-byte aligned and every period is 1 or a multiple of 4 with a 16-byte aligned base, 4-byte accesses otherwise; the results do
 * not depend on which. */
int be_lif_syn_sg_forward_params(const float* x, const float* c0, const float* v0, const float* a0, const float* syn_decay,
                                 int64_t sd_period, const float* beta, int64_t beta_period, const float* v_th, int64_t vth_period,
                                 const float* rho, int64_t rho_period, const float* kappa, int64_t kappa_period, float* s_out,
                                 float* v_seq, float* h_save, float* c_save, float* a_save, float* c_last, float* v_last,
                                 float* a_last, int64_t T, int64_t N, double v_reset, int reset_mode, int adaptive,
                                 be_stream_t stream);
int be_lif_syn_sg_backward_params(const float* h_save, const float* c_save, const float* a_save, const float* c0, const float* v0,
                                  const float* g_s, const float* g_vseq, const float* g_clast, const float* g_vlast,
                                  const float* g_alast, const float* syn_decay, int64_t sd_period, const float* beta,
                                  int64_t beta_period, const float* v_th, int64_t vth_period, const float* rho, int64_t rho_period,
                                  const float* kappa, int64_t kappa_period, float* g_x, float* g_c0, float* g_v0, float* g_a0,
                                  float* g_sd_slot, float* g_beta_slot, float* g_vth_slot, float* g_rho_slot, float* g_kappa_slot,
                                  int64_t T, int64_t N, double v_reset, int reset_mode, int surrogate, double alpha, int adaptive,
                                  int detach_reset, be_stream_t stream);
/* The recurrent spiking layer (brainevent_amd/csrc/be_neuron_sg_rec.hip): the neuron above with a CSR recurrence INSIDE the time
 * loop — step t's input is x[t] + s[t-1] @ W_rec.  One launch forwards, one backwards; one workgroup per sample.  x, s_out, v_seq,
 * h_save, th_save, g_s, g_vseq, g_x are [T, B, N] row-major; s0, c0, v0, a0, the *_last, g_c0, g_v0, g_a0, g_s0 are [B, N].  The
 * matrix is CSR [N, N], rows = presynaptic neurons: w (f32, one per stored entry), indices (int32 columns), indptr (int32 [N + 1]);
 * duplicate columns in a row, self-loops and empty rows are allowed.  scale_exp = e is the fixed-point exponent of the sums
 * (be_fixed_point_exponent's bound — every row active — is this kernel's worst case): scale = ldexpf(1, e - 32), inv = ldexp(1.0, -e).
 *   forward, for every sample b independently, t = 0 .. T-1, sp = s0[b] (NULL: no spike) before step 0 and s_out[t-1][b] after it:
 *     R[j] = sum over the stored entries k whose row i has sp[i] != 0 and whose column is j of fixed(w[k])
 *            fixed(w): t = w * scale;  hf = floor(t);  ((int64)(int32)hf << 32) | (uint32)((t - hf) * 2^32)
 *            (a 64-bit wrapping integer sum: order independent)
 *     r[j] = (float)((double)(int64)R[j] * inv)
 *     xin  = x[t][b][j] + r[j]              (one rounded f32 addition; when no row is active r = +0 and the addition is still made)
 *     then the forward step above, verbatim, with xin in the place of x[t][i]
 *   The forward pass is therefore a function of its inputs, bit for bit.
 *   backward, t = T-1 .. 0, the carries cc, cv, ca as above; G[.] = g_x[t+1][b][.], which the previous iteration produced:
 *     g_rec = t < T-1 ? sum over the entries k of row i of w[k] * G[indices[k]] : not used
 *             (each product rounded, then summed in f32 in an order the row's length alone fixes: lane j of 16 takes the entries
 *             j, j + 16, ... in order, then a butterfly over the 16 partial sums)
 *     g_sp  = g_s[t][b][i] (NULL: 0);   if t < T-1: g_sp = g_sp + g_rec;   then the backward step above continues unchanged
 *             (adaptive: + ca; the reset term unless detach_reset; g_u, g_h, g_c; g_x[t][b][i] = g_c; the three carries)
 *   after the loop g_c0, g_v0, g_a0 as above;  g_s0[b][i] = sum over row i of w[k] * g_x[0][b][indices[k]]   (if given)
 *   g_x[t] is the gradient of x[t] and of r[t] alike (straight-through in the spikes, as the event-driven products); detach_reset
 *   does not cut the recurrent path.  The weight gradient is be_grad_rows (transpose = 1) over the T * B batch rows
 *   sp[t][b] / g_x[t][b], with g_sn = 1, g_sb = N.
 * T == 0, B == 0 or N == 0: BE_OK, nothing launched.  BE_ERR_RANGE: N > 8192 (one sample's sums and spike ids live in one
 * workgroup's LDS).  BE_ERR_INVALID: the codes above; B < 0; w, indices or indptr NULL; scale_exp outside -90 .. 150 (what
 * be_fixed_point_exponent returns).  Every index must lie in [0, N).  No global atomics; never synchronises the host. */
int be_lif_rec_sg_forward(const float* x, const float* w, const int32_t* indices, const int32_t* indptr, const float* s0,
                          const float* c0, const float* v0, const float* a0, float* s_out, float* v_seq, float* h_save,
                          float* th_save, float* c_last, float* v_last, float* a_last, int64_t T, int64_t B, int64_t N,
                          double syn_decay, double beta, double v_th, double v_reset, double rho, double kappa, int reset_mode,
                          int adaptive, int scale_exp, be_stream_t stream);
int be_lif_rec_sg_backward(const float* h_save, const float* th_save, const float* w, const int32_t* indices, const int32_t* indptr,
                           const float* g_s, const float* g_vseq, const float* g_clast, const float* g_vlast, const float* g_alast,
                           float* g_x, float* g_c0, float* g_v0, float* g_a0, float* g_s0, int64_t T, int64_t B, int64_t N,
                           double syn_decay, double beta, double v_th, double v_reset, double rho, double kappa, int reset_mode,
                           int surrogate, double alpha, int adaptive, int detach_reset, be_stream_t stream);
/* The recurrent layer with syn_decay, beta, v_th, rho and kappa read from DEVICE memory (the same kernels, csrc/be_neuron_sg_rec.hip;
 * the reduce is be_lif_sg_reduce_slots above, called once per parameter that needs a gradient, with N' = B * N and P = N or 1).  Each
 * of the five is an f32 array with a period of its own, which is 1 (one value for the layer) or N (one per neuron, shared by the
 * samples of the batch: the layer's neurons are the same neurons in every sample, as the matrix is); neuron i uses
 * param[period == 1 ? 0 : i] — write sd_i, beta_i, vth_i, rho_i, kappa_i.  v_reset and alpha stay host scalars.  Arrays and shapes
 * as be_lif_rec_sg_forward / _backward; c_save and a_save are [T, B, N], the five slot arrays [B, N].
 *   forward, for every sample b, t = 0 .. T-1: R[j], r[j] and xin = x[t][b][j] + r[j] exactly as be_lif_rec_sg_forward (the wrapping
 *   64-bit fixed-point sum, r = (float)((double)(int64)R * inv), one rounded addition), then the step of
 *   be_lif_syn_sg_forward_params, verbatim, with neuron i's own five values and xin in the place of x[t][i]:
 *     a_in = a;  c = (sd_i * c) + xin;  h = (beta_i * v) + c;  th = adaptive ? vth_i + (kappa_i * a_in) : vth_i;  s = h >= th;
 *     v = hard: s ? v_reset : h   soft: s ? h - vth_i : h;   a = adaptive ? (rho_i * a_in) + (s ? 1 : 0)
 *     s_out, v_seq, h_save as there;  c_save[t][b][i] = c (if given);  a_save[t][b][i] = a_in (adaptive and h_save given)
 *   a_save takes the place of th_save and c_save is needed for g_sd_slot alone, as there.
 *   backward, t = T-1 .. 0: g_rec, g_sp = g_s[t][b][i] (+ g_rec if t < T-1), g_x and g_s0 exactly as be_lif_rec_sg_backward, the
 *   step that of be_lif_syn_sg_backward_params with the recomputed th, and its five accumulators per (sample, neuron), each +0 at
 *   t = T-1, added to in descending t, every operation rounded on its own, each kept only if its output pointer is given:
 *     acc_sd    = acc_sd    + (g_c * c_prev)          c_prev = t > 0 ? c_save[t-1][b][i] : c0[b][i]   (NULL: 0)
 *     acc_beta  = acc_beta  + (g_h * v_prev)          v_prev = t > 0 ? membrane_after(h_save[t-1][b][i], th_prev, vth_i, v_reset)
 *                                                              : v0[b][i]   (NULL: 0),  th_prev from a_save[t-1][b][i]
 *     d = g_u;  soft only: d = d + (s ? g_vo : 0);    acc_vth = acc_vth - d
 *     acc_kappa = acc_kappa - (g_u * a_in)            (adaptive)
 *     acc_rho   = acc_rho   + (ca_in * a_in)          (adaptive; ca_in: the trace's carry BEFORE this step updates it)
 *   after the loop g_sd_slot[b][i], g_beta_slot[b][i], g_vth_slot[b][i], g_rho_slot[b][i], g_kappa_slot[b][i] hold them.  The
 *   kernel keeps each accumulator IN its output entry (read, add, write by the one thread that owns the entry, plain vector loads
 *   and stores, no atomics): the additions and their order are the ones written here, so the bits are a register accumulator's.
 *   c0 and c_save are read only when g_sd_slot is given, v0 only when g_beta_slot is.
 * T == 0, B == 0 or N == 0: BE_OK, nothing launched.  BE_ERR_RANGE: N > 8192.  BE_ERR_INVALID: everything be_lif_rec_sg_forward /
 * _backward and be_lif_syn_sg_forward_params / _backward_params refuse, and a period that is neither 1 nor N.  With adaptive == 0 the
 * adaptation's pointers and periods are neither read nor written.  No global atomics; never synchronises the host. */
int be_lif_rec_sg_forward_params(const float* x, const float* w, const int32_t* indices, const int32_t* indptr, const float* s0,
                                 const float* c0, const float* v0, const float* a0, const float* syn_decay, int64_t sd_period,
                                 const float* beta, int64_t beta_period, const float* v_th, int64_t vth_period, const float* rho,
                                 int64_t rho_period, const float* kappa, int64_t kappa_period, float* s_out, float* v_seq,
                                 float* h_save, float* c_save, float* a_save, float* c_last, float* v_last, float* a_last, int64_t T,
                                 int64_t B, int64_t N, double v_reset, int reset_mode, int adaptive, int scale_exp,
                                 be_stream_t stream);
int be_lif_rec_sg_backward_params(const float* h_save, const float* c_save, const float* a_save, const float* c0, const float* v0,
                                  const float* w, const int32_t* indices, const int32_t* indptr, const float* g_s,
                                  const float* g_vseq, const float* g_clast, const float* g_vlast, const float* g_alast,
                                  const float* syn_decay, int64_t sd_period, const float* beta, int64_t beta_period,
                                  const float* v_th, int64_t vth_period, const float* rho, int64_t rho_period, const float* kappa,
                                  int64_t kappa_period, float* g_x, float* g_c0, float* g_v0, float* g_a0, float* g_s0,
                                  float* g_sd_slot, float* g_beta_slot, float* g_vth_slot, float* g_rho_slot, float* g_kappa_slot,
                                  int64_t T, int64_t B, int64_t N, double v_reset, int reset_mode, int surrogate, double alpha,
                                  int adaptive, int detach_reset, be_stream_t stream);
/* The recurrent layer with SYNAPTIC DELAYS (brainevent_amd/csrc/be_neuron_sg_rec_delay.hip): be_lif_rec_sg_forward / _backward with
 * the stacked matrix of a delay split in the place of the CSR matrix.  w, indices (int32 columns in [0, N)) and indptr (int32
 * [depth * N + 1]) are the STACKED arrays: stacked row d * N + i holds the stored entries of presynaptic neuron i whose conduction
 * delay is d steps, 0 <= d < depth <= 256 (be_delay_split_count / _fill produce them).  row_mask (uint32 [depth, ceil(N / 32)], bit
 * i % 32 of word i / 32 of row d set where stacked row d * N + i is NOT empty; NULL keeps every row) lets both passes skip empty
 * stacked rows; it must not clear the bit of a row that has entries, and the results do not depend on whether it is given.
 * s_hist / g_s_hist are [hist_ages, B, N], 0 <= hist_ages <= depth: s_hist[a] are the spikes emitted a + 1 steps before step 0
 * (active where != 0); ages from hist_ages on are silent.  Every other array, shape and scalar is be_lif_rec_sg_forward /
 * _backward's.  Write sp(tau)[b][i] = s_out[tau][b][i] != 0 for tau >= 0, s_hist[-1 - tau][b][i] != 0 for -hist_ages <= tau < 0,
 * false below.
 *   forward, for every sample b independently, t = 0 .. T-1:
 *     R[j] = sum over the stored entries k of every ACTIVE stacked row whose column is j of fixed(w[k]);  stacked row d * N + i is
 *            active when sp(t - 1 - d)[b][i]     (fixed() and the 64-bit wrapping integer sum as be_lif_rec_sg_forward: order
 *            independent)
 *     r[j] = (float)((double)(int64)R[j] * inv);   xin = x[t][b][j] + r[j]   (one rounded f32 addition, made even when r = +0)
 *     then the forward step of be_lif_syn_sg_forward, verbatim, with xin in the place of x[t][i]
 *   The forward pass is therefore a function of its inputs, bit for bit; depth = 1 is be_lif_rec_sg_forward with s0 = s_hist[0].
 *   backward, t = T-1 .. 0, the carries cc, cv, ca as there; g_x[t + 1 ..] are what the earlier iterations produced:
 *     g_rec = +0;  for d = 0, 1, .. ascending while d < depth and t + 1 + d <= T-1:
 *               g_rec = g_rec + (sum over the entries k of stacked row d * N + i of w[k] * g_x[t + 1 + d][b][indices[k]])
 *             (each product rounded; the row sum in f32 in an order the row's length alone fixes: lane j of 2 takes the entries
 *             j, j + 2, ... in order from +0, then the two partial sums are added; an empty row adds +0)
 *     g_sp  = g_s[t][b][i] (NULL: 0);   if t < T-1: g_sp = g_sp + g_rec;   then the backward step continues unchanged
 *   after the loop g_c0, g_v0, g_a0 as there, and, if g_s_hist is given, for a < hist_ages:
 *     g_s_hist[a][b][i] = +0, then for d = a, a + 1, .. ascending while d < depth and d - a <= T-1:
 *               + (sum over the entries k of stacked row d * N + i of w[k] * g_x[d - a][b][indices[k]])     (the same row sum)
 *   g_x is a REQUIRED output: it is the history the gathers read back (the workgroup's own stores, ordered by workgroup barriers).
 *   Two calls on the same inputs give identical bits.  The weight gradient is be_grad_rows (transpose = 1) over the stacked matrix
 *   (n_rows = depth * N) and the T * B batch rows (t, b) of g_x, g_sn = 1, g_sb = N, with the activity mask of
 *   be_grad_pack_activity_aged below: g_w[k] = sum over (t, b) ascending of sp(t - 1 - d)[b][i] * g_x[t][b][indices[k]].
 * LIMITS: N <= 8192 and 8 * N + 8 * depth * ceil(N / 64) + 16384 <= 162816 bytes (one sample's sums, its spike history and a list
 * of at least 4096 active rows live in one workgroup's LDS): every N <= 8192 with depth <= 16 and every N <= 2048 with depth <= 256
 * fit.  BE_ERR_RANGE beyond them, by both calls.  T == 0, B == 0 or N == 0: BE_OK, nothing launched.  BE_ERR_INVALID: depth outside
 * 1 .. 256; hist_ages outside 0 .. depth; hist_ages > 0 with s_hist NULL (forward); g_x NULL; everything be_lif_rec_sg_forward /
 * _backward list.  No global atomics, no workspace; never synchronises the host. */
int be_lif_rec_delay_sg_forward(const float* x, const float* w, const int32_t* indices, const int32_t* indptr, const uint32_t* row_mask,
                                int depth, const float* s_hist, int hist_ages, const float* c0, const float* v0, const float* a0,
                                float* s_out, float* v_seq, float* h_save, float* th_save, float* c_last, float* v_last, float* a_last,
                                int64_t T, int64_t B, int64_t N, double syn_decay, double beta, double v_th, double v_reset, double rho,
                                double kappa, int reset_mode, int adaptive, int scale_exp, be_stream_t stream);
int be_lif_rec_delay_sg_backward(const float* h_save, const float* th_save, const float* w, const int32_t* indices,
                                 const int32_t* indptr, const uint32_t* row_mask, int depth, const float* g_s, const float* g_vseq,
                                 const float* g_clast, const float* g_vlast, const float* g_alast, float* g_x, float* g_c0, float* g_v0,
                                 float* g_a0, float* g_s_hist, int hist_ages, int64_t T, int64_t B, int64_t N, double syn_decay,
                                 double beta, double v_th, double v_reset, double rho, double kappa, int reset_mode, int surrogate,
                                 double alpha, int adaptive, int detach_reset, be_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * event vector helpers (replace: brainevent/_jit_scalar/binary_jitsmv.cu:107-125 `_pack_bool_kern`
 * and the active-row extraction of brainevent/_csr/binary_csrmv_hybrid.cu:275-327)
 * ---------------------------------------------------------------------------------------------- */
/* spikes[n] -> bits[ceil(n/32)] (bit i%32 of word i/32 set iff spike i active) */
int be_pack_spikes(const void* spikes, int spike_dtype, int64_t n, uint32_t* bits, be_stream_t stream);
/* batch-major spikes_bm[n_batch, n] -> bits[n_batch, ceil(n/32)] */
int be_pack_spikes_batched(const void* spikes_bm, int spike_dtype, int64_t n, int64_t n_batch, uint32_t* bits,
                           be_stream_t stream);
/* bits[ceil(n/32)] -> spikes_out[n] (one 0/1 byte per spike) */
int be_unpack_spikes(const uint32_t* bits, int64_t n, uint8_t* spikes_out, be_stream_t stream);
/* spikes[n] -> active_ids[<=n] (unordered) and *count (device uint32) */
int be_compact_spikes(const void* spikes, int spike_dtype, int64_t n, uint32_t* active_ids, uint32_t* count,
                      be_stream_t stream);
/* batch-major spikes_bm[n_batch, n] -> active_ids[b * active_stride + ...] and counts[b] */
int be_compact_spikes_batched(const void* spikes_bm, int spike_dtype, int64_t n, int64_t n_batch, uint32_t* active_ids,
                              int64_t active_stride, uint32_t* counts, be_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * spike exchange of the multi-GPU partition (the reference has no distributed path): one process per
 * GPU, rank g owns a post slice of the matrix and the spikes of its 1/G of the pre population; ONE all-gather of the
 * bit-packed slices (RCCL over xGMI) rebuilds the full spike vector on every rank, which the scatter entry points consume
 * as it is (BE_SPIKE_BITS).  Every rank owns the same whole number of 32-bit words: slice of rank r =
 * [r * w * 32, (r + 1) * w * 32) clipped to n_pre, w = ceil(ceil(n_pre / 32) / world) (be_exchange_slice).
 *   rank 0: be_exchange_get_unique_id(id)  ->  the binder ships the be_exchange_unique_id_bytes() bytes to every process
 *   all   : be_exchange_init(id, world, rank, n_pre, &ex)        (collective: ncclCommInitRank; current HIP device)
 *   step  : be_exchange_allgather_bits(ex, local_spikes, dtype, full_bits, stream)   full_bits: be_exchange_full_words(ex) words
 *           dtype BE_SPIKE_BITS: local_spikes are the slice's own words (bits past the slice 0): a slice that fills its w words
 *           is gathered from where it lies (no pack launch, no copy); with be_exchange_post the words must stay unchanged
 *           until the slot's be_exchange_wait has been queued
 *   end   : be_exchange_destroy(ex)
 * The handle owns the communicator and one device buffer of w words.  RCCL is loaded with dlopen("librccl.so") on first use
 * (override: environment variable BE_RCCL_LIB); BE_ERR_UNSUPPORTED if it cannot be loaded.
 * ---------------------------------------------------------------------------------------------- */
int be_exchange_unique_id_bytes(void);
int be_exchange_get_unique_id(void* id_host);
int be_exchange_init(const void* id_host, int world, int rank, int64_t n_pre, void** exchange_host_out);
int be_exchange_slice(const void* exchange, int rank, int64_t* lo_host, int64_t* hi_host);
/* the same partition as a pure function (no handle, no device, no RCCL): rank's slice [lo, hi) of n_pre spikes and the words
 * every rank owns — what init, slice, allgather and post all compute; any of the three outputs may be NULL */
int be_exchange_slice_for(int64_t n_pre, int world, int rank, int64_t* lo_host, int64_t* hi_host, int64_t* words_per_rank_host);
int64_t be_exchange_full_words(const void* exchange);
int be_exchange_allgather_bits(void* exchange, const void* local_spikes, int spike_dtype, uint32_t* full_bits,
                               be_stream_t stream);
/* pipelined form (synaptic delays >= 2 steps): post step t + 1's exchange on the library's own stream — it waits for what
 * producer_stream has queued so far, i.e. the spikes — then scatter step t; wait makes consumer_stream wait for the posted
 * slot (0 / 1, alternate them) and returns its device buffer, valid until that slot is posted again.
 * Slot reuse: the gather into a slot must not start before the consumer's last read of the slot's previous contents.  When
 * consumer_stream IS producer_stream (one stream issues the scatters and the posts) that order is implied: post waits for
 * everything that stream has queued.  A consumer on another stream calls be_exchange_release(ex, slot, consumer_stream)
 * after queueing its last read of the slot; the next post into the slot then waits for that point too.
 * A failed be_exchange_post (stream / event / buffer creation) leaves the handle usable: the next call starts over. */
int be_exchange_post(void* exchange, const void* local_spikes, int spike_dtype, int slot, be_stream_t producer_stream);
int be_exchange_wait(void* exchange, int slot, const uint32_t** full_bits_out, be_stream_t consumer_stream);
int be_exchange_release(void* exchange, int slot, be_stream_t consumer_stream);
/* The posted exchange that ALSO compacts what it gathered: right behind the all-gather, still on the library's own stream, the
 * slot's words become the list of active pre neurons (ids + a device counter, as be_compact_spikes writes them).
 * be_exchange_wait_ids makes consumer_stream wait for the slot and fills *ids_out — pass a pointer to it as the `spikes` argument
 * of a scatter entry point with spike dtype BE_SPIKE_IDS (n_batch = 1): the scatter then runs no compaction of its own, fused or
 * launched, on the consumer's critical path.  *full_bits_out (optional) = the slot's words, as be_exchange_wait returns them.
 * Same slot, lifetime and release rules as be_exchange_post / _wait; the list holds up to n_pre ids and lives in the handle.
 * The exchange's events are created without a system-scope fence (they order work of one device; environment variable
 * BE_EXCHANGE_SYSTEM_FENCE=1 restores default events). */
int be_exchange_post_ids(void* exchange, const void* local_spikes, int spike_dtype, int slot, be_stream_t producer_stream);
int be_exchange_wait_ids(void* exchange, int slot, be_spike_ids_t* ids_out, const uint32_t** full_bits_out,
                         be_stream_t consumer_stream);
/* Measurement hook (process-wide; also environment variable BE_EXCHANGE_EMULATE_US at start-up): every all-gather issued from now on
 * is followed, on its own stream, by a spin kernel of `us` microseconds — a stand-in for the latency of a real multi-rank all-gather
 * on a box with one GPU, so that the sequential and the pipelined schedule can be timed against an exchange of realistic length
 * (bench.py rank_breakdown.emulated).  0 switches it off (the default). */
int be_exchange_emulate_latency_us(double us);
int be_exchange_destroy(void* exchange);

/* ------------------------------------------------------------------------------------------------
 * Batch convention (all *mm entry points): spikes_bm is batch-major [n_batch, len] and out_bm is
 * batch-major [n_batch, out_len] — the physical layout the reference's SRAW kernels also emit
 * (brainevent/_csr/binary.py:1263-1286, brainevent/_fcn/binary.py:867-889: "Python transposes back").
 * The *mv entry points are the n_batch = 1 case of the same kernels.
 * ---------------------------------------------------------------------------------------------- */

/* ------------------------------------------------------------------------------------------------
 * binary_csrmv / binary_csrmm, transpose=True (scatter):  out[indices[j]] += w[j]  for every active row
 * replaces: binary_csrmv_wat_hybrid_{homo,hetero}_{f32,f64,f16,bf16}_{bool,float}
 *           (brainevent/_csr/binary_csrmv_hybrid.cu:619-632, 789-821),
 *           binary_csrmm_sraw_hybrid_{…} (brainevent/_csr/binary_csrmm_hybrid.cu:16-57, 469-530)
 * and, with indptr == NULL and row_len = n_conn, binary_fcnmv_scatter_{…} / binary_fcnmm_sraw_{…}
 *           (brainevent/_fcn/binary_fcnmv.cu:55-137, 207-217; brainevent/_fcn/binary_fcnmm.cu:486-529, 835-857).
 *   weights : [nnz] (hetero) or [1] (homo), dtype wdtype;  out : [n_batch, k] dtype wdtype (fully written)
 *   spikes  : [n_batch, m];  indices : [nnz] int32 in [0,k);  indptr : [m+1] or NULL (rows are row_len long)
 *   workspace : >= be_binary_csrmm_t_workspace_bytes(m, k, n_batch, wdtype) bytes, 256-byte aligned
 * "direct" route: no preprocessing, global float atomics.
 * ---------------------------------------------------------------------------------------------- */
int64_t be_binary_csrmv_t_workspace_bytes(int64_t m, int64_t k, int wdtype);
int64_t be_binary_csrmm_t_workspace_bytes(int64_t m, int64_t k, int64_t n_batch, int wdtype);
int be_binary_csrmv_t(const void* weights, int homo, int wdtype, const int32_t* indices, const void* indptr,
                      int indptr_is_i64, int64_t row_len, const void* spikes, int spike_dtype, void* out,
                      int64_t m, int64_t k, void* workspace, int64_t workspace_bytes, be_stream_t stream);
int be_binary_csrmm_t(const void* weights, int homo, int wdtype, const int32_t* indices, const void* indptr,
                      int indptr_is_i64, int64_t row_len, const void* spikes_bm, int spike_dtype, void* out_bm,
                      int64_t m, int64_t k, int64_t n_batch, void* workspace, int64_t workspace_bytes,
                      be_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * post-sliced scatter plan (the MI355X-native layout behind `spk @ CSR` / `spk @ FixedNumPerPre`).
 * Plays the role of the reference's per-matrix task workspace
 * (brainevent/_csr/main.py:58-88, brainevent/_csr/hybrid_config.py:298-324): built once per matrix,
 * cached by the CSR object, passed to every call.
 *
 * Layout: output neurons are cut into slices of `slice_width` columns (slice = column / slice_width, local column =
 * column % slice_width); 2^slice_shift is the accumulator capacity of a workgroup (LDS) and the stride of its
 * partial sums, slice_width <= 2^slice_shift, and slice_width = 0 means 2^slice_shift.  A width below the capacity
 * balances the slices (k = 1M, shift 14: 64 slices of 15625 instead of 61 full ones and a sliver of 576).
 * For row r and slice s the entries of row r
 * whose column falls in slice s form one 128-byte-aligned block inside `blob`:
 *     hetero: [ f32 weight x 4*ng ][ uint16 local column x 4*ng ]   with ng = ceil(count / 4) lane groups
 *     homo  : [ uint16 local column x 8*ng ]                          with ng = ceil(count / 8)
 * pads carry local column 2^slice_shift (a dummy accumulator) and weight 0.
 *     seg[(r * n_slices + s)] = { uint32 block start in 128-B units, uint32 ng }     (8 bytes per entry)
 * layout BE_PLAN_D8 (heterogeneous weights, at most 1024 slices, rows of at most 16384 entries — be_scatter_plan_count
 * checks every row on the device and returns BE_ERR_RANGE for a longer one): 5 bytes per entry —
 *     block: [ f32 weight x 4*ng ][ uint8 delta x 4*ng ], entries sorted by column, column = previous column + delta
 *     (first delta 0), gaps above 255 bridged by escape entries (weight 0, delta 255), tail pads (weight 0, delta 0);
 *     seg = { block start in 128-B units, ng | (local column of the first entry << 16) }.
 * layout BE_PLAN_H8 (one homogeneous weight; same limits as d8; slice_width up to 40000): 1 byte per entry —
 *     block: [ uint8 code x 8*ng ], entries sorted by column; code c < 255: advance c columns and count one entry,
 *     c = 255: advance 255 columns and count nothing (a gap g is g / 255 escapes followed by the code g % 255; tail pads
 *     are 255); the first code is 0 and seg is as for d8.
 *
 *   step 1  be_scatter_plan_count : fills seg (m * n_slices entries of 8 B) and returns the size of `blob`
 *           in *blob_bytes_host.  SYNCHRONOUS (it reads the total back).
 *   step 2  caller allocates blob (128-byte aligned, blob_bytes + 128).
 *   step 3  be_scatter_plan_fill  : fills blob; writes the f32 bit patterns of max |w| and of the smallest non-zero |w|
 *           to maxabs_bits[0] and maxabs_bits[1] (device uint32[2]) so that the caller can pick the fixed-point exponent
 *           and refuse matrices whose dynamic range the 64-bit fixed-point sums cannot resolve.
 *   later   be_scatter_plan_refresh_weights : same arguments as the fill, over the SAME seg / blob, after the weights of
 *           an unchanged structure were updated (plasticity).  The reference's cached workspace holds task ranges only
 *           (brainevent/_csr/main.py:58-88, :148-161), so weight updates never invalidate it; here the blocks embed the
 *           weights, and this call is what keeps them current.  Re-derive scale_exp from the new maxabs / column sums.
 * ---------------------------------------------------------------------------------------------- */
#define BE_BINNED_ACC32 2 /* `homo` argument of the binned entry points: per-entry weights, 32-bit fixed-point sums */
#define BE_BINNED_ABS 4   /* ... OR-ed to 0 / 2: the step sums |w| (column statistics: how a caller derives scale_exp with a few
                            binned steps over all the rows instead of a pass of global atomics over the entries) */
#define BE_BINNED_SHORT_ROWS 8 /* ... OR-ed to any kind, a performance hint for matrices WITH an indptr: the stored rows average at
                                 most 256 entries (pass B keeps one step of loads in flight instead of two; rows of one length —
                                 indptr NULL — are classified by row_len).  Results do not depend on it. */
#define BE_BINNED_OUT_F32 16 /* ... OR-ed to any kind: `out` is f32 [n_batch, k] whatever the weight dtype.  The sums are accumulated
                                 in f32 and, without this flag, rounded once to f16 / bf16 weights' own dtype; column statistics
                                 (BE_BINNED_ABS) need them unrounded — 8 significant bits lose more than the exponent's 1.001 margin. */
#define BE_PLAN_U16 0 /* uint16 local columns (both weight kinds) */
#define BE_PLAN_D8 1  /* sorted columns as uint8 deltas (heterogeneous weights) */
#define BE_PLAN_H8 2  /* sorted columns as uint8 advance codes (one homogeneous weight) */
int64_t be_scatter_plan_scratch_bytes(int64_t m, int64_t k, int slice_shift, int slice_width);
int be_scatter_plan_count(const int32_t* indices, const void* indptr, int indptr_is_i64, int64_t row_len,
                          int64_t m, int64_t k, int slice_shift, int slice_width, int homo, int layout, void* seg,
                          void* scratch, int64_t scratch_bytes, int64_t* blob_bytes_host, be_stream_t stream);
int be_scatter_plan_fill(const void* weights, int homo, int wdtype, const int32_t* indices, const void* indptr,
                         int indptr_is_i64, int64_t row_len, int64_t m, int64_t k, int slice_shift, int slice_width,
                         int layout, const void* seg, void* blob, uint32_t* maxabs_bits, be_stream_t stream);
int be_scatter_plan_refresh_weights(const void* weights, int homo, int wdtype, const int32_t* indices, const void* indptr,
                                    int indptr_is_i64, int64_t row_len, int64_t m, int64_t k, int slice_shift,
                                    int slice_width, int layout, const void* seg, void* blob, uint32_t* maxabs_bits,
                                    be_stream_t stream);
/* Planning a matrix from BLOCKS OF ROWS that are resident one at a time (a matrix whose raw CSR and plan do not fit the device
 * together).  Everything the count and the fill touch is local to a row except the block starts, which one scan over the whole
 * segment table provides:
 *   be_scatter_plan_begin(m, k, ...)                                once: scratch as for be_scatter_plan_count, whole matrix
 *   be_scatter_plan_count_rows(block, ..., m_rows, m_total, ..., seg + r0 * n_slices * 8 bytes, scratch, ..., order_blk)   per block:
 *                          indices / indptr of rows [r0, r0 + m_rows), indptr RELATIVE to the block (indptr[0] == 0)
 *   be_scatter_plan_scan(m, k, ..., seg, scratch, ..., &blob_bytes)   once, SYNCHRONOUS; the caller allocates blob
 *   be_scatter_plan_fill_ordered(block, ..., m = m_rows, ..., seg + r0 * n_slices * 8, blob, maxabs, order_blk)           per block;
 *                          every call restarts maxabs: combine the blocks' (max, min) on the caller's side
 * be_scatter_plan_count[_ordered] is exactly begin + count_rows over all rows + scan. */
int be_scatter_plan_begin(int64_t m, int64_t k, int slice_shift, int slice_width, void* scratch, int64_t scratch_bytes,
                          be_stream_t stream);
int be_scatter_plan_count_rows(const int32_t* indices, const void* indptr, int indptr_is_i64, int64_t row_len, int64_t m_rows,
                               int64_t m_total, int64_t k, int slice_shift, int slice_width, int homo, int layout, void* seg_rows,
                               void* scratch, int64_t scratch_bytes, uint16_t* order_out, be_stream_t stream);
int be_scatter_plan_scan(int64_t m, int64_t k, int slice_shift, int slice_width, void* seg, void* scratch, int64_t scratch_bytes,
                         int64_t* blob_bytes_host, be_stream_t stream);

/* The sorted layouts (BE_PLAN_D8 / BE_PLAN_H8) need every row in column order.  The *_ordered forms keep that order instead of
 * sorting three times: the count pass writes it — order[nnz] uint16, the row-local position of the i-th smallest column of
 * each row — and the fill and every later weight refresh read it back (a gather-copy: no sort).  order == NULL, or the
 * BE_PLAN_U16 layout: exactly the calls above.  The caller may free `order` after the fill (the build then saved one sort)
 * or keep it — 2 bytes per stored entry — for as long as it wants cheap refreshes. */
int be_scatter_plan_count_ordered(const int32_t* indices, const void* indptr, int indptr_is_i64, int64_t row_len, int64_t m,
                                  int64_t k, int slice_shift, int slice_width, int homo, int layout, void* seg, void* scratch,
                                  int64_t scratch_bytes, int64_t* blob_bytes_host, uint16_t* order_out, be_stream_t stream);
int be_scatter_plan_fill_ordered(const void* weights, int homo, int wdtype, const int32_t* indices, const void* indptr,
                                 int indptr_is_i64, int64_t row_len, int64_t m, int64_t k, int slice_shift, int slice_width,
                                 int layout, const void* seg, void* blob, uint32_t* maxabs_bits, const uint16_t* order,
                                 be_stream_t stream);
int be_scatter_plan_refresh_weights_ordered(const void* weights, int homo, int wdtype, const int32_t* indices, const void* indptr,
                                            int indptr_is_i64, int64_t row_len, int64_t m, int64_t k, int slice_shift,
                                            int slice_width, int layout, const void* seg, void* blob, uint32_t* maxabs_bits,
                                            const uint16_t* order, be_stream_t stream);

/* Plastic plans: a plan of per-entry f32 / f16 / bf16 weights (BE_PLAN_U16 / BE_PLAN_D8) kept current under in-place weight
 * updates (be_plasticity_rows) with work proportional to the entries the update touched.  None of these calls computes weight
 * statistics, takes an exponent or synchronises: the caller runs its steps at a scale_exp that the weights cannot outgrow
 * (bounds [w_min, w_max] that the update clips to: scale_exp <= 62 - ceil(log2(cmax * max(|w_min|, |w_max|))), cmax = the most
 * stored entries on one output column).  All launches go to `stream`, so a captured step replays them.
 *
 * be_scatter_plan_refresh_rows : the update was row-driven (perm == NULL there).  The blocks — entries, escapes, tail pads — of
 *   every ACTIVE stored row are rewritten exactly as be_scatter_plan_fill_ordered writes them; `order` (or NULL: the rows are
 *   sorted again) as there.  spikes / spike_dtype: any encoding be_plasticity_rows takes (a spike is any nonzero value), over
 *   the m stored rows; an id list (BE_SPIKE_IDS) holds ids below m, each at most once — the contract of be_plasticity_rows,
 *   whose list this is; the same holds for the ids below k of be_scatter_plan_patch_entries (they index t_indptr).  slot: NULL, or the table below — the refreshed rows' entries are
 *   rewritten (BE_PLAN_U16 draws block positions from a counter, so a refresh moves them).
 *   workspace >= be_scatter_plan_refresh_workspace_bytes(m).
 * be_scatter_plan_slots : builds slot[nnz] (uint16): the position of raw entry j inside its (row, slice) block.  It rewrites
 *   every block from `weights` on the way (for BE_PLAN_U16 positions and columns are only consistent with the pass that drew
 *   them).  Fits uint16 by the layouts' limits: a d8 block holds at most 16384 entries + slice_width / 255 escapes; for
 *   BE_PLAN_U16 the caller guarantees rows of at most 65536 entries (checked where row_len says so: BE_ERR_RANGE).
 * be_scatter_plan_patch_entries : the update went through the transposed structure (t_indptr[k + 1], t_rows[nnz], perm[nnz]:
 *   for every secondary id the stored rows holding it and the raw positions of those entries).  For every entry e of every
 *   ACTIVE secondary id c it stores (float)weights[perm[e]] at
 *   blob + (seg[t_rows[e] * n_slices + c / slice_width].start << 7) + 4 * slot[perm[e]].  spikes: over the k secondary ids.
 *   workspace >= be_scatter_plan_refresh_workspace_bytes(k). */
int64_t be_scatter_plan_refresh_workspace_bytes(int64_t n);
int be_scatter_plan_refresh_rows(const void* weights, int wdtype, const int32_t* indices, const void* indptr, int indptr_is_i64,
                                 int64_t row_len, int64_t m, int64_t k, int slice_shift, int slice_width, int layout,
                                 const void* seg, void* blob, const uint16_t* order, uint16_t* slot, const void* spikes,
                                 int spike_dtype, void* workspace, int64_t workspace_bytes, be_stream_t stream);
int be_scatter_plan_slots(const void* weights, int wdtype, const int32_t* indices, const void* indptr, int indptr_is_i64,
                          int64_t row_len, int64_t m, int64_t k, int slice_shift, int slice_width, int layout, const void* seg,
                          void* blob, const uint16_t* order, uint16_t* slot, be_stream_t stream);
int be_scatter_plan_patch_entries(const void* weights, int wdtype, const void* t_indptr, int t_indptr_is_i64,
                                  const int32_t* t_rows, const void* perm, int perm_is_i64, int64_t nnz, const uint16_t* slot,
                                  int64_t m, int64_t k, int slice_shift, int slice_width, int layout, const void* seg, void* blob,
                                  const void* spikes, int spike_dtype, void* workspace, int64_t workspace_bytes,
                                  be_stream_t stream);

/* Fixed-point exponent of a weight array — the `scale_exp` of the planned and the binned step — chosen by the library:
 *   overflow bound : the largest e with (largest column sum of |w|) * 2^e < 2^62 (every row active; a row may list a column
 *                    several times, so "rows x max|w|" is NOT a bound).  indices == NULL: all the weights bound a column.
 *   accuracy gate  : e is accepted when the largest weight of every non-empty output column keeps `min_weight_bits` bits
 *                    (16 gives ~1e-5 of the column's weight scale, the tolerance of the path).
 *   keep_exp       : an exponent to keep when it still cannot overflow (weights refreshed under a captured graph, where
 *                    scale_exp is a recorded launch argument), or INT_MIN.
 * SYNCHRONOUS (reads statistics back).  Returns BE_ERR_RANGE — use the direct route — for inf / nan weights or a dynamic
 * range 64-bit sums cannot resolve.  scratch >= be_fixed_point_scratch_bytes(k).  Every index must lie in [0, k): the passes
 * address colsum[indices[j]] unchecked.  No reference counterpart: its GPU kernels add floats with global atomics
 * (brainevent/_csr/binary_csrmv_hybrid.cu:199-234).
 *   the bound      : 1.001 x the largest f32 column sum S', summed with float atomics.  Every add rounds by at most half an ulp,
 *                    i.e. 2^-24 of the running sum, which never exceeds S' (the addends are non-negative): the true sum S of a
 *                    column of n entries obeys S <= S' (1 + n 2^-24).  The step wraps at 2^63, the rule keeps 1.001 S' 2^e below
 *                    2^62: that spare bit covers S <= 2.002 S', i.e. any column of up to n = 2^24 entries (1.68e7), whatever its
 *                    weights.  (Equal weights are the worst case: their sum stops growing at 2^24 addends, the next one being
 *                    exactly half an ulp, so such a column stays safe up to 1.001 x 2^25 entries and wraps beyond.)  Past that
 *                    in-degree take the plan's exponent, whose sums are integers.  A column sum beyond the f32 range (inf) is
 *                    replaced by max|w| * (nnz + 1) in f64, always valid: such weights are not refused. */
int64_t be_fixed_point_scratch_bytes(int64_t k);
/* max |w| and the smallest non-zero |w| of a weight array as f32 bit patterns (0 / 0xffffffff when there is none; a max at or
 * above 0x7f800000 means inf / nan): one streaming pass.  scratch >= 256 bytes.  SYNCHRONOUS. */
int be_weight_stats(const void* weights, int wdtype, int64_t n, uint32_t* max_bits_host, uint32_t* min_nonzero_bits_host,
                    void* scratch, int64_t scratch_bytes, be_stream_t stream);
int be_fixed_point_exponent(const void* weights, int wdtype, const int32_t* indices, int64_t nnz, int64_t k,
                            int min_weight_bits, int keep_exp, void* scratch, int64_t scratch_bytes, int* scale_exp_host,
                            be_stream_t stream);
/* The same exponent — same gate and keep_exp rule — for a matrix that has a WEIGHTED plan (BE_PLAN_U16 with per-entry
 * weights, BE_PLAN_D8), computed from the plan's own blocks: one workgroup per slice sums |w| of every row's block in LDS
 * (64-bit fixed point, addends rounded up: the bound never falls short) — a planned step with all rows active — instead of two
 * passes of global float atomics over the raw entries (1e10 entries: 0.47 s -> tens of ms).  Its bound is the sum itself, without
 * the entry pass's 1.001 margin: the result equals be_fixed_point_exponent's or is ONE ABOVE it (largest column sum within 0.1 %
 * under a power of two); away from the clamps it is never below.  Both are safe.  maxabs_bits: what be_scatter_plan_fill left.
 * min_weight_bits: 0 ... 40.  scratch >= 256 bytes.  SYNCHRONOUS. */
int be_scatter_plan_exponent(const void* blob, const void* seg, int64_t m, int64_t k, int slice_shift, int slice_width, int layout,
                             int64_t nnz, const uint32_t* maxabs_bits, int min_weight_bits, int keep_exp, void* scratch,
                             int64_t scratch_bytes, int* scale_exp_host, be_stream_t stream);

/* planned scatter step: out[n_batch, k] (dtype wdtype, fully written) from spikes[n_batch, m].
 *   weights : device pointer to weights[0] (homo only; may be NULL for hetero)
 *   scale_exp : fixed-point exponent chosen by the caller (hetero only): every stored weight is accumulated as
 *               round(w * 2^scale_exp) in a 64-bit integer (order independent, bitwise reproducible).  The largest
 *               column sum of |w| times 2^scale_exp must stay below 2^62 (a row may list a column several times, so
 *               "rows x max|w|" is NOT a bound); sums that exceed it wrap silently.
 *   block_hint : average stored items per (row, slice) block of the plan — nnz / (m * slices); for BE_PLAN_D8 the
 *               entries plus its escape items, i.e. 4 x the average of the table's lane-group counts — or 0 (unknown).
 *               A speed hint only, never a correctness input: short blocks are decoded by 4, 8 or 16 lanes each instead
 *               of a wave each (the variant whose single pass holds the average + 3 sigma of a Poisson length; longer
 *               blocks finish in a serial tail), and with >= 40 slices of blocks <= 64 items the step first gathers the
 *               active rows' table entries into the workspace (two small launches more).
 *   parts : number of workgroups that share one slice (each takes 1/parts of the active rows)
 *   workspace : >= be_binary_csrmm_t_plan_workspace_bytes(m, k, n_batch, slice_shift, slice_width, parts, homo) bytes
 *               (spike counters + active-row list + partial sums; for a single vector and >= 40 slices also room for the
 *               pre-gathered segment table, 8 B x m x slices, up to 8 GiB).
 *               Its first 4 * n_batch bytes (the spike counters) must be ZERO on entry; they are zero again when the
 *               call has completed, so a workspace zero-filled once can be reused for every step.
 */
int64_t be_binary_csrmv_t_plan_workspace_bytes(int64_t m, int64_t k, int slice_shift, int slice_width, int parts, int homo);
int64_t be_binary_csrmm_t_plan_workspace_bytes(int64_t m, int64_t k, int64_t n_batch, int slice_shift, int slice_width,
                                               int parts, int homo);
/* the same plus room for the pre-gathered segment table, which the single-vector step uses for plans of >= 40 slices and short
 * blocks (block_hint <= 64, the value passed to the step): without it the step gathers from the plan's own table (correct,
 * slower there); with a block_hint that does not qualify the two sizes are equal */
int64_t be_binary_csrmm_t_plan_workspace_bytes_for(int64_t m, int64_t k, int64_t n_batch, int slice_shift, int slice_width,
                                                   int parts, int homo, int block_hint);
int be_binary_csrmv_t_plan(const void* weights, int homo, int wdtype, const void* blob, const void* seg,
                           const void* spikes, int spike_dtype, void* out, int64_t m, int64_t k, int slice_shift,
                           int slice_width, int layout, int block_hint, int parts, int scale_exp, void* workspace,
                           int64_t workspace_bytes, be_stream_t stream);
int be_binary_csrmm_t_plan(const void* weights, int homo, int wdtype, const void* blob, const void* seg,
                           const void* spikes_bm, int spike_dtype, void* out_bm, int64_t m, int64_t k, int64_t n_batch,
                           int slice_shift, int slice_width, int layout, int block_hint, int parts, int scale_exp,
                           void* workspace, int64_t workspace_bytes, be_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * binned scatter: the event-driven transpose=True product for a matrix WITHOUT a plan (raw CSR / fixed-length rows),
 * f32 / f16 / bf16 weights.  Pass B: 256 workgroups stream the active rows' entries, four per lane and load, and append
 * each to a write-combining block of its output slice ("bin") in LDS (two blocks of 8 ... 128 entries per bin; a ticket
 * per entry, one commit per entry, no workgroup barrier); a completed block is copied to the workgroup's own region of
 * the bin — no global atomics.  Pass C: one workgroup per bin streams the bin's 256 regions and accumulates in LDS
 * (integer atomics, like the planned route).  A region that overflows its share of `bin_capacity` is delivered through
 * global float atomics into an overflow image of the output instead (slower, still correct: pass C adds the image in), so
 * `bin_capacity` is a tuning parameter, not a correctness one:
 * about 1.5 x expected_active_rows x mean_row_length / be_binned_bins(k, slice_shift, homo).  The library cuts the k outputs
 * into a multiple of 256 bins of equal width (one workgroup per bin in pass C, 256 CUs), as few as one bin's accumulators fit
 * LDS and at most 2^slice_shift columns wide (slice_shift in [4, 16]; 16 = as wide as LDS allows); be_binned_bins returns
 * that count, or 0 when pass B's LDS cannot hold two blocks per bin (more than 2048 / 1146 bins counted / weighted).
 * A column index >= k is the caller's error (the entry is dropped).
 * Reproducibility: sums are integers (counts, or 64-bit fixed point at 2^scale_exp) converted once, so the result is
 * bitwise identical from call to call as long as (i) no region overflows and (ii) the matrix has more than 128 bins
 * (k > 32768: one workgroup per bin).  With fewer bins several workgroups share a bin and
 * merge through float atomics, and an overflowing block is added with float atomics too: both are order dependent in
 * the last bit (still within the 1e-5 tolerance of the path).  The planned route has neither exception.
 * Same role as binary_csrmv_wat_hybrid_* (brainevent/_csr/binary_csrmv_hybrid.cu:619-632): no preprocessing.
 * `homo` of the binned entry points names the KIND of a step: 0 = per-entry weights, sums in 64-bit fixed point at 2^scale_exp;
 * 1 = one shared weight (counts); BE_BINNED_ACC32 (2) = per-entry weights, sums in 32-bit fixed point at 2^scale_exp — bins twice
 * as wide (10M outputs: 256 bins, one round of pass C, instead of 611), for matrices whose every column keeps its largest weight
 * at >= 18 bits at that exponent: scale_exp = be_fixed_point_exponent(..., min_weight_bits = 18 + 32, ...) - 32 (BE_ERR_RANGE:
 * use kind 0).  The largest column sum of |w| times 2^scale_exp stays below 2^30 by the same call; sums stay integers
 * (order independent).  be_binned_bins and the workspace sizes take the same kind (a workspace is sized for all three).
 * ---------------------------------------------------------------------------------------------- */
int be_binned_bins(int64_t k, int slice_shift, int homo);
/* Task size of pass B (process-wide, read at every call): a task is about task_groups groups of four consecutive entries — but at
 * least four rows while those stay within 1024 groups —, and a step is cut into at least min_tasks tasks.  Defaults 256 / 2048
 * (measured on gfx950; rounds 1-3: 1024 / 2048); the Python layer sets them from its
 * persisted per-architecture tuning — the counterpart of the thresholds the reference compiles into its hybrid kernel from
 * brainevent/_csr/hybrid_config.py:77-88, :256-295. */
int be_binned_set_tuning(int task_groups, int min_tasks);
/* Sticky protocol flag of a binned workspace.  Pass B's append never blocks for good: a lane whose write-combining slot is not
 * freed within 20 ms (constant-rate clock; never observed) raises the flag and drops its pending entries, pass C then writes
 * NaN into every output of that step — the process keeps its HIP context (the reference's device-side check traps instead,
 * brainevent/include/brainevent/check.h:79-82).  This call reads the flag: BE_OK, or BE_ERR_HIP with the cause in
 * be_last_error(); clear != 0 re-arms the workspace.  SYNCHRONOUS.  A caller that never sees NaN never needs it.
 * The same call checks the workspace's CONSERVATION COUNTERS (four uint64 that every step adds to; be_binned_workspace_audit reads
 * them): [0] stored entries of the active rows (from the row bounds), [1] tickets pass B drew, [2] entries pass C added to its
 * accumulators, [3] entries delivered through the overflow image.  After complete steps [0] == [1] == [2] + [3]; otherwise
 * BE_ERR_RANGE with the four numbers in be_last_error() — an entry was lost or delivered twice (or a column id is >= k: the
 * caller's error, dropped by pass B, shows as [0] > [1]).  clear != 0 zeroes the counters too.  The reference has no counterpart:
 * its scatter adds with global atomics (brainevent/_csr/binary_csrmv_hybrid.cu:330-350), nothing is staged that could be lost. */
int be_binned_workspace_status(const void* workspace, int clear, be_stream_t stream);
/* the four conservation counters of a binned workspace -> counters_host[4].  SYNCHRONOUS. */
int be_binned_workspace_audit(const void* workspace, uint64_t* counters_host, be_stream_t stream);
int64_t be_binary_csrmv_t_binned_workspace_bytes(int64_t m, int64_t k, int slice_shift, int64_t bin_capacity);
/* once per workspace, before its first step: zeroes the spike counter and the overflow image inside it (every step leaves
 * both at zero, so the step itself needs no memset and no zeroing of `out`: pass C writes every output) */
int be_binary_csrmv_t_binned_workspace_init(void* workspace, int64_t workspace_bytes, int64_t m, int64_t k, int slice_shift,
                                            int64_t bin_capacity, be_stream_t stream);
int be_binary_csrmv_t_binned(const void* weights, int homo, int wdtype, const int32_t* indices, const void* indptr,
                             int indptr_is_i64, int64_t row_len, const void* spikes, int spike_dtype, void* out,
                             int64_t m, int64_t k, int slice_shift, int64_t bin_capacity, int scale_exp, void* workspace,
                             int64_t workspace_bytes, be_stream_t stream);
/* the same for a batch: spikes_bm [n_batch, m] (bit-packed: [n_batch, ceil(m / 32)] words), out_bm [n_batch, k].  The rows with a
 * spike in ANY batch row are read once for up to 32 batch rows at a time — each entry is appended once per batch row that has
 * its row active, into that batch row's own bins — as long as pass B's LDS holds blocks for all their bins (wide bins: few
 * per batch row); otherwise one single-vector step per batch row, as the reference's batched scatter does
 * (brainevent/_csr/binary_csrmm_hybrid.cu:16-57, brainevent/_fcn/binary_fcnmm.cu:486-529).  `bin_capacity` as for one vector. */
int64_t be_binary_csrmm_t_binned_workspace_bytes(int64_t m, int64_t k, int64_t n_batch, int slice_shift, int64_t bin_capacity);
int be_binary_csrmm_t_binned_workspace_init(void* workspace, int64_t workspace_bytes, int64_t m, int64_t k, int64_t n_batch,
                                            int slice_shift, int64_t bin_capacity, be_stream_t stream);
int be_binary_csrmm_t_binned(const void* weights, int homo, int wdtype, const int32_t* indices, const void* indptr,
                             int indptr_is_i64, int64_t row_len, const void* spikes_bm, int spike_dtype, void* out_bm,
                             int64_t m, int64_t k, int64_t n_batch, int slice_shift, int64_t bin_capacity, int scale_exp,
                             void* workspace, int64_t workspace_bytes, be_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * binary_csrmv / binary_csrmm, transpose=False (gather):  out[i] = sum_j w[j] * e(spikes[indices[j]])
 * replaces: binary_csrmv_nt_auto_{homo,hetero}_{…}_{bool,float} (brainevent/_csr/binary_csrmv.cu:437-486),
 *           binary_csrmm_nt_auto_{…} (brainevent/_csr/binary_csrmm.cu:328-392) and, with indptr == NULL,
 *           the gather direction of binary_fcnmv / binary_fcnmm (brainevent/_fcn/binary.py:201-253, 731-766).
 *   spikes : [n_batch, k];  out : [n_batch, m];  workspace >= be_binary_csrmm_nt_workspace_bytes(m, k, n_batch)
 * ---------------------------------------------------------------------------------------------- */
int64_t be_binary_csrmv_nt_workspace_bytes(int64_t m, int64_t k);
int64_t be_binary_csrmm_nt_workspace_bytes(int64_t m, int64_t k, int64_t n_batch);
int be_binary_csrmv_nt(const void* weights, int homo, int wdtype, const int32_t* indices, const void* indptr,
                       int indptr_is_i64, int64_t row_len, const void* spikes, int spike_dtype, void* out,
                       int64_t m, int64_t k, void* workspace, int64_t workspace_bytes, be_stream_t stream);
int be_binary_csrmm_nt(const void* weights, int homo, int wdtype, const int32_t* indices, const void* indptr,
                       int indptr_is_i64, int64_t row_len, const void* spikes_bm, int spike_dtype, void* out_bm,
                       int64_t m, int64_t k, int64_t n_batch, void* workspace, int64_t workspace_bytes,
                       be_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * CSR -> CSC structure conversion in column blocks, on the device, 64-bit offsets (no entry-count limit).
 * replaces: csr_to_csc_count / csr_to_csc_fill_block (brainevent/_csr/csr_to_csc.cu:137-199) and the host loop around them
 *           (brainevent/_misc.py:1380-1513 `_csr_to_csc_index_gpu_column_block`; public entry brainevent/_misc.py:1516
 *           `csr_to_csc_index(..., method="gpu_column_block")`), `fixed_conn_num_csc_structure` (brainevent/_misc.py:1255,
 *           with indptr == NULL and row_len = n_conn).  It is what the mirror of the unfavourable direction is built from
 *           (brainevent/_csr/main.py:1321-1357 `_weight_indices`, brainevent/_fcn/main.py:280-300).
 *   1  be_csr_to_csc_count   : counts[n_cols] (int64) <- stored entries per column (one pass over `indices`)
 *   2  be_csr_to_csc_indptr  : exclusive scan -> csc_indptr[n_cols + 1] (int64 or int32); *nnz_host (may be NULL; when given
 *                              the call is SYNCHRONOUS; BE_ERR_RANGE if an int32 indptr cannot hold the total)
 *   3  be_csr_to_csc_fill_block, once per column block [col_lo, col_hi), any partition of the columns: the block's entries go to
 *        rows_out / weights_out / perm_out — arrays of the BLOCK (csc_indptr[col_hi] - csc_indptr[col_lo] elements), slot =
 *        csc_indptr[column] - csc_indptr[col_lo] + position inside the column.  csc_indptr is the int64 form of step 2.
 *        rows_out: the row of every entry (int32);  weights_out: its weight, moved along (weight_bytes = 2 / 4 / 8, or 0: no
 *        weights — one shared weight);  perm_out: its position in the CSR arrays (int32 or int64; NULL = not wanted: 8 bytes
 *        per entry is more than the structure itself).  cursor: scratch of (col_hi - col_lo) int64.
 *   The order of the entries INSIDE a column is unspecified (slots are drawn from per-column cursors with atomics), exactly as
 *   in the reference's kernel (csr_to_csc.cu:26-27); every product over the result is insensitive to it.
 *   be_gather_by_perm: out[i] = src[perm[i]] for 2 / 4 / 8-byte elements — how a mirror that kept perm follows a weight update.
 *   be_csr_to_csc_fill_block_u8: step 3 with a ONE-byte payload per entry (bytes[nnz] -> bytes_out, both non-NULL): how the FP8
 *        codes of a Float8CSR move into its mirror.  Everything else as be_csr_to_csc_fill_block, which keeps refusing a
 *        weight_bytes of 1.
 * ---------------------------------------------------------------------------------------------- */
int64_t be_csr_to_csc_scratch_bytes(int64_t n_cols);
int be_csr_to_csc_count(const int32_t* indices, int64_t nnz, int64_t n_cols, int64_t* counts, be_stream_t stream);
int be_csr_to_csc_indptr(const int64_t* counts, int64_t n_cols, void* csc_indptr_out, int out_is_i64, int64_t* nnz_host,
                         void* scratch, int64_t scratch_bytes, be_stream_t stream);
int be_csr_to_csc_fill_block(const int32_t* indices, const void* indptr, int indptr_is_i64, int64_t row_len, int64_t m,
                             int64_t nnz, int64_t col_lo, int64_t col_hi, const int64_t* csc_indptr, int64_t* cursor,
                             int32_t* rows_out, void* perm_out, int perm_is_i64, const void* weights, int weight_bytes,
                             void* weights_out, be_stream_t stream);
int be_csr_to_csc_fill_block_u8(const int32_t* indices, const void* indptr, int indptr_is_i64, int64_t row_len, int64_t m,
                                int64_t nnz, int64_t col_lo, int64_t col_hi, const int64_t* csc_indptr, int64_t* cursor,
                                int32_t* rows_out, void* perm_out, int perm_is_i64, const void* bytes, void* bytes_out,
                                be_stream_t stream);
int be_gather_by_perm(const void* src, int elem_bytes, const void* perm, int perm_is_i64, int64_t n, void* out,
                      be_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * float-operand twins (last clause): the same CSR / fixed-number matrices against a dense vector or matrix.
 * replaces: csrmv / csrmm (brainevent/_csr/float.py:49-150, :559-668; CPU loops :153-207, :670-744; float_csrmv.cu,
 *           float_csrmm.cu) and fcnmv / fcnmm (brainevent/_fcn/float.py:33-134, :136-240) — indptr NULL + row_len = n_conn.
 *   transpose = 0:  out[i, c] = sum over row i of w_j * B[indices[j], c]            B [k, n], out [m, n]   (one writer per row)
 *   transpose = 1:  out[indices[j], c] += w_j * B[i, c] for every stored row i      B [m, n], out [k, n]   (float atomics)
 * B, out and the weights share wdtype (f32 / f64 / f16 / bf16; sums in f32 / f64); row-major, n >= 1 (be_csrmv: n = 1).
 * homo != 0: one shared weight weights[0] (the sum is multiplied once, like the reference's `w * r`).  indices and per-entry
 * weights must be 16-byte aligned (rows are read in aligned groups of four).  nnz_hint: the stored entries if the caller knows
 * them (it selects the lanes per row; 0 = unknown).  workspace: be_csrmm_workspace_bytes (an f32 image of the output for the
 * f16 / bf16 scatter; 256 bytes otherwise).  Zeros of the operand are skipped in the scatter direction (they add nothing).
 * ---------------------------------------------------------------------------------------------- */
int64_t be_csrmm_workspace_bytes(int64_t m, int64_t k, int64_t n, int transpose, int wdtype);
int be_csrmm(const void* weights, int homo, int wdtype, const int32_t* indices, const void* indptr, int indptr_is_i64,
             int64_t row_len, const void* B, void* out, int64_t m, int64_t k, int64_t n, int64_t nnz_hint, int transpose,
             void* workspace, int64_t workspace_bytes, be_stream_t stream);
int be_csrmv(const void* weights, int homo, int wdtype, const int32_t* indices, const void* indptr, int indptr_is_i64,
             int64_t row_len, const void* v, void* out, int64_t m, int64_t k, int64_t nnz_hint, int transpose, void* workspace,
             int64_t workspace_bytes, be_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * per-synapse products ("dt2t"): one output per stored entry, the entry's value times a per-neuron factor — the D^t e^{t-1}
 * term of an eligibility-trace update, or any per-synapse state scaled per neuron.
 * replaces: csrmv_dt2t / csrmm_dt2t / cscmv_dt2t / cscmm_dt2t (brainevent/_csr/dt2t.py:42-234, :545-760; _csr/dt2t.cu)
 *           and fcnmv_dt2t / fcnmm_dt2t (brainevent/_fcn/dt2t.py:33-345) — indptr NULL + row_len = n_conn.
 *   by_col = 0:  out[b, j] = w[b, j] * y[b, row(j)]        y [n_batch, n_rows]
 *   by_col = 1:  out[b, j] = w[b, j] * y[b, indices[j]]    y [n_batch, n_cols]
 * w, out [n_batch, nnz] and y share wdtype (f32 / f64 / f16 / bf16); the product is formed in f32 (f64 for f64) and rounded
 * once.  homo != 0: w is one shared value w[0] for every batch row.  out is written in full; out == w (in place) is allowed.
 * indptr (by_col = 0 only; ignored otherwise) must ascend from 0 to nnz over n_rows + 1 entries; indptr NULL: row r holds
 * entries [r * row_len, (r + 1) * row_len).  indices is read only when by_col != 0 (may be NULL otherwise).  No pointer needs
 * more than its element's alignment: the runs that hang over a 16-byte boundary are handled in the kernel.  No workspace,
 * nothing allocated, no host synchronisation: capturable in a HIP graph.  nnz = 0 or n_batch = 0 returns without a launch;
 * n_batch <= 65535.  Entry offsets are 64-bit throughout.
 * ---------------------------------------------------------------------------------------------- */
int be_dt2t(const void* w, int homo, int wdtype, const void* y, const int32_t* indices, const void* indptr, int indptr_is_i64,
            int64_t row_len, void* out, int64_t n_rows, int64_t n_cols, int64_t n_batch, int64_t nnz, int by_col,
            be_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * row slicing: rows of a stored matrix as a dense block (W[rows]), the gradient of that read, and the sparse sub-matrix.
 * replaces: csr_slice_rows / csr_slice_rows_grad (brainevent/_csr/slice.py:39-120, :300-365; slice_csr_slice_rows.cu) and the
 *           host-side gather of build_sub_csr (brainevent/_misc.py:1199-1252) — indptr NULL + row_len = n_conn for the
 *           fixed-number containers.  rows / urows / ks / seg / new_indptr are int64.
 *   be_slice_rows:       out[k, c] = sum of data[j] over the entries j of row rows[k] with indices[j] == c; out [n_sel, n_cols],
 *                        contiguous, wdtype, EVERY element written (no memset needed; rows of out may start off 16 bytes).  A
 *                        row index outside [0, n_rows) gives a zero row.  Duplicates of a column are added in ascending j, in
 *                        f32 (f64 for f64), one rounding; homo != 0: out = (number of entries on the column) * data[0], one
 *                        product (+0 where there is none, whatever the sign of data[0]).  No float atomics: bit-reproducible.  Cost: ceil(n_cols / be_slice_rows_tile_cols) passes
 *                        over each selected row.
 *   be_slice_rows_grad:  dw[j] = sum over k with rows[k] == row(j) of ct[k, indices[j]], ascending k, f32 (f64), one rounding;
 *                        zero for entries of rows not selected (the entry point fills dw itself, on the stream).  The caller
 *                        groups the selection: urows [n_u] the distinct rows, seg [n_u + 1] the offsets of each one's k's in
 *                        ks [n_sel] (ascending k inside a row).  Rows outside [0, n_rows) contribute nothing.  homo != 0:
 *                        dw [1] = the sum over everything: one partial per distinct row in workspace
 *                        (be_slice_rows_grad_workspace_bytes), then one workgroup sums them in a fixed order.  No atomics.
 *   be_slice_rows_copy:  out_indices[new_indptr[k] + i] = indices[indptr[rows[k]] + i] (and data alike when data != NULL,
 *                        elem_bytes 2 / 4 / 8) for every selected row; new_indptr [n_sel + 1] is the prefix sum of the selected
 *                        rows' lengths, new_nse its last element.  Balanced per entry.
 * ---------------------------------------------------------------------------------------------- */
int be_slice_rows_tile_cols(int wdtype);
int be_slice_rows(const void* data, int homo, int wdtype, const int32_t* indices, const void* indptr, int indptr_is_i64,
                  int64_t row_len, const int64_t* rows, int64_t n_sel, void* out, int64_t n_rows, int64_t n_cols, int64_t nse,
                  be_stream_t stream);
int64_t be_slice_rows_grad_workspace_bytes(int64_t n_sel, int wdtype);
int be_slice_rows_grad(const void* ct, int wdtype, const int32_t* indices, const void* indptr, int indptr_is_i64, int64_t row_len,
                       const int64_t* urows, const int64_t* seg, const int64_t* ks, int64_t n_u, int64_t n_sel, void* dw, int homo,
                       int64_t n_rows, int64_t n_cols, int64_t nse, void* workspace, int64_t workspace_bytes, be_stream_t stream);
int be_slice_rows_copy(const int32_t* indices, const void* data, int elem_bytes, const void* indptr, int indptr_is_i64,
                       int64_t row_len, const int64_t* rows, const int64_t* new_indptr, int64_t n_sel, int64_t n_rows, int64_t nse,
                       int64_t new_nse, int32_t* out_indices, void* out_data, be_stream_t stream);

/* JIT connectivity against a dense operand: the same on-the-fly matrices as be_binary_jitmv / be_binary_jitmm (same walks, same
 * per-edge weight hashes), every element of the operand counting.
 * replaces: jitsmv / jitsmm (brainevent/_jit_scalar/float.py:838-905, :1331-1420), jitumv / jitumm, jitnmv / jitnmm
 *           (brainevent/_jit_uniform/float.py, brainevent/_jit_normal/float.py).
 *   X [in_len, n] -> out [out_len, n], row-major, wdtype = the weight dtype (sums in float64 for the gather orientation, f32 /
 *   f64 atomics for the scatter orientation).  stride: 32 = the matrix a vector operand sees, 4 = the matrix a matrix operand
 *   sees (the reference draws them differently; be_jitmv_float: n = 1, stride 32).  gather != 0: generator rows = outputs
 *   (corder = True), else generator rows = inputs.  mode / w0 / w1 / clen / seed / shape1 as be_binary_jitmv. */
int64_t be_jitmm_float_workspace_bytes(int64_t shape1, int64_t in_len, int64_t out_len, int64_t n, int gather, int wdtype);
int be_jitmm_float(int mode, double w0, double w1, int wdtype, int64_t clen, uint32_t seed, const void* X, void* out, int64_t shape1,
                   int64_t in_len, int64_t out_len, int64_t n, int stride, int gather, void* workspace, int64_t workspace_bytes,
                   be_stream_t stream);
/* The scatter orientation (gather = 0) through LDS fixed-point sums instead of float atomics — the event-driven scatter's structure
 * with the operand's value as a per-row factor (C3 shape, dense operand: the walk's rate instead of 21 G atomics/s).  BATCH-major
 * operand X_bm [n, in_len] and result out_bm [n, out_len]; scale_exp such that |w|max * |x|max * in_len * 2^scale_exp < 2^62 —
 * the caller knows the operand's largest magnitude.  f32 / f16 / bf16 (f64 operands: be_jitmm_float, whose atomics are f64). */
int64_t be_jitmm_float_scatter_workspace_bytes(int64_t shape1, int64_t out_len, int64_t n, int stride);
int be_jitmm_float_scatter(int mode, double w0, double w1, int wdtype, int64_t clen, uint32_t seed, const void* X_bm, void* out_bm,
                           int64_t shape1, int64_t in_len, int64_t out_len, int64_t n, int stride, int scale_exp, void* workspace,
                           int64_t workspace_bytes, be_stream_t stream);
int be_jitmv_float(int mode, double w0, double w1, int wdtype, int64_t clen, uint32_t seed, const void* v, void* out, int64_t shape1,
                   int64_t in_len, int64_t out_len, int gather, void* workspace, int64_t workspace_bytes, be_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * perm-fused ("indexed") products: be_binary_csrmm_{t,nt} over a RE-INDEXED structure whose slot j carries
 * weights[perm[j]] — the weights stay in their canonical order and only the weights of active rows (t) / of entries whose
 * input fired (nt) are read; no data[perm] pass per call.
 * replaces: binary_indexed_csrmv_hybrid / binary_indexed_csrmm_hybrid (brainevent/_csr/binary_indexed_csrmv_hybrid.cu:16-23,
 *           brainevent/_csr/binary_indexed.py:70, :615).  perm: [nnz] int32 or int64; homo != 0 or perm == NULL: the plain
 *           product (one shared weight ignores perm, as in the reference).  Workspaces as for be_binary_csrmm_{t,nt}.
 * These are the preprocessing-free forms (global atomics / one wave per row).  A structure that is used every step is
 * planned once from the permuted weights instead (be_scatter_plan_*), after which a step reads no weight array at all.
 * ---------------------------------------------------------------------------------------------- */
int be_binary_csrmm_t_indexed(const void* weights, int homo, int wdtype, const int32_t* indices, const void* indptr,
                              int indptr_is_i64, int64_t row_len, const void* perm, int perm_is_i64, const void* spikes_bm,
                              int spike_dtype, void* out_bm, int64_t m, int64_t k, int64_t n_batch, void* workspace,
                              int64_t workspace_bytes, be_stream_t stream);
int be_binary_csrmm_nt_indexed(const void* weights, int homo, int wdtype, const int32_t* indices, const void* indptr,
                               int indptr_is_i64, int64_t row_len, const void* perm, int perm_is_i64, const void* spikes_bm,
                               int spike_dtype, void* out_bm, int64_t m, int64_t k, int64_t n_batch, void* workspace,
                               int64_t workspace_bytes, be_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * binary_densemv / binary_densemm  (BinaryArray @ ndarray)
 * replaces: binary_densemv_{transpose,no_transpose}_{f32..bf16}_{bool,float} (brainevent/_dense/binary_densemv.cu:52-149),
 *           binary_densemm_{transpose,no_transpose}_{…} (brainevent/_dense/binary_densemm.cu:50-162) and the cuBLAS
 *           variants binary_dense{mv,mm}_cublas_{nt,t}_f32_bool (brainevent/_dense/binary_dense_cublas.cu:139-212).
 *   weights : [rows_w, cols_w] row-major, dtype wdtype
 *   transpose = 1: spikes_bm [n_batch, rows_w] -> out_bm [n_batch, cols_w],  out[b, j] = sum_{i: e(s[b,i])} W[i, j]
 *   transpose = 0: spikes_bm [n_batch, cols_w] -> out_bm [n_batch, rows_w],  out[b, i] = sum_{j: e(s[b,j])} W[i, j]
 *   workspace >= be_binary_densemm_workspace_bytes(rows_w, cols_w, n_batch, transpose, wdtype)
 * Sums are accumulated in f32 (f64 for f64 weights) in a fixed order: results are reproducible.
 * ---------------------------------------------------------------------------------------------- */
int64_t be_binary_densemm_workspace_bytes(int64_t rows_w, int64_t cols_w, int64_t n_batch, int transpose, int wdtype);
int be_binary_densemm(const void* weights, int wdtype, const void* spikes_bm, int spike_dtype, void* out_bm,
                      int64_t rows_w, int64_t cols_w, int64_t n_batch, int transpose, void* workspace,
                      int64_t workspace_bytes, be_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * The same products with OCP FP8 weights, one byte per weight (brainevent_amd/csrc/be_dense_f8.hip; no counterpart in the
 * reference).  f8_format: BE_F8_E4M3 (torch.float8_e4m3fn) or BE_F8_E5M2 (torch.float8_e5m2); never the fnuz forms.
 *   weights : [rows_w, cols_w] row-major codes
 *   transpose = 1: spikes_bm [n_batch, rows_w] -> out_f32_bm [n_batch, cols_w],  out[b, j] = fl32((sum_{i: e(s[b,i])} W[i, j]) * scale)
 *   transpose = 0: spikes_bm [n_batch, cols_w] -> out_f32_bm [n_batch, rows_w],  out[b, i] = fl32((sum_{j: e(s[b,j])} W[i, j]) * scale)
 *   scale   : one number per matrix, rounded to f32 once and applied to the finished f32 sum (scale = 1 leaves it bit for bit)
 *   workspace >= be_binary_densemm_f8_workspace_bytes(rows_w, cols_w, n_batch, transpose, f8_format)
 * The output is always f32.  spike_dtype: BE_SPIKE_BOOL, BE_SPIKE_FLOAT or BE_SPIKE_BITS.  Same contracts as be_binary_densemm
 * (contraction dimension < 2^28; a contraction of length 0 gives zeros; empty outputs return BE_OK; asynchronous on `stream`,
 * no host read, capturable), sums in f32 in a fixed order.
 * PRECONDITION: every code is finite (e4m3: (c & 0x7f) != 0x7f; e5m2: (c & 0x7c) != 0x7c) — a non-finite code in a row that
 * carries a spike makes every batch row of its MFMA tile NaN, and there is no repair pass.
 * ---------------------------------------------------------------------------------------------- */
#define BE_F8_E4M3 0
#define BE_F8_E5M2 1
int64_t be_binary_densemm_f8_workspace_bytes(int64_t rows_w, int64_t cols_w, int64_t n_batch, int transpose, int f8_format);
int be_binary_densemm_f8(const void* weights, int f8_format, double scale, const void* spikes_bm, int spike_dtype,
                         void* out_f32_bm, int64_t rows_w, int64_t cols_w, int64_t n_batch, int transpose, void* workspace,
                         int64_t workspace_bytes, be_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * FP8 weights for the event-driven CSR products: `events @ W8`, the scatter over the active rows of a CSR matrix whose stored
 * entries are OCP FP8 codes, one byte each (brainevent_amd/csrc/be_csr_f8.hip, the q8 layout of be_csr_plan.hip; no counterpart
 * in the reference).  FP8 is not a wdtype: the format travels as f8_format (BE_F8_E4M3 / BE_F8_E5M2, never the fnuz forms).
 *
 * Semantics.  E = 9 for e4m3 and 16 for e5m2; Q(c) = decode(c) * 2^E is an exact integer for every finite code c
 * (|Q| <= 229 376 for e4m3, <= 3 758 096 384 for e5m2).  For output column j of batch row b:
 *     R_j    = sum over the active rows i of b, over the stored entries e of row i with indices[e] == j, of Q(codes[e])   (int64, exact)
 *     out[j] = (float)((double)(long long)R_j * inv),      inv = ldexp((double)(float)scale, -E)
 * "Active" is the rule of every scatter entry point: BE_SPIKE_BOOL != 0, BE_SPIKE_FLOAT > 0 (a negative or NaN value is
 * inactive), a set bit of BE_SPIKE_BITS, a listed id of BE_SPIKE_IDS (single vector).  The output is always f32; there is one f32
 * scale per matrix.  (double)R_j is exact while |R_j| < 2^53, and R_j itself cannot overflow while a column has fewer than 2^31
 * stored entries (2^31 * 3 758 096 384 < 2^63).  The sums are integers at a fixed exponent: no per-matrix exponent, no accuracy gate,
 * and the result is bit-identical whatever the route (plan or direct), the slice geometry, `parts` or the order of the adds.
 * PRECONDITION: every code is finite (e4m3: (c & 0x7f) != 0x7f; e5m2: (c & 0x7c) != 0x7c); the kernels do not test it.
 *
 * Common contracts: explicit stream, caller-owned buffers, nothing allocated, no host read in a step (capturable); m, k or
 * n_batch of zero: BE_OK and nothing else done, after the scalar arguments were checked.  BE_ERR_INVALID: an unknown f8_format or
 * spike dtype, a non-finite scale, negative sizes, m or k above 2^32 - 1, n_batch above 65535, a NULL buffer, slice_shift outside
 * [4, 15], slice_width negative or above max(2^slice_shift, 20000), parts outside [1, 64].  BE_ERR_WORKSPACE: a workspace or scratch
 * that is NULL or too small.  BE_ERR_UNSUPPORTED: BE_SPIKE_IDS with n_batch > 1.
 *
 * Direct route: compaction, then a lane group per active row adds Q into int64[n_batch, k] with global 64-bit integer atomics,
 * then one convert kernel.  No layout and no limits on rows or slices.  nnz = stored entries (sizes the lane group: a speed hint
 * when indptr is given).  indptr == NULL: rows of row_len entries.
 *   workspace >= be_binary_csrmm_t_f8_workspace_bytes(m, k, n_batch)
 *
 * Planned route, layout "q8": 2 bytes per entry.  For row r and slice s (slices as for the plans above) one 128-byte-aligned block
 *     [ uint8 code x 4*ng ][ uint8 delta x 4*ng ],   seg = { block start in 128-B units, ng | (local column of the first entry << 16) }
 * with the entries sorted by column and BE_PLAN_D8's delta rules: column = previous column + delta (first delta 0), a gap above
 * 255 bridged by escape entries (code 0x00, delta 255), tail pads (code 0, delta 0).  Limits as d8: rows of at most 16384 entries
 * (be_scatter_plan_q8_count checks every row on the device: BE_ERR_RANGE for a longer one), at most 1024 slices and a slice whose
 * 64-bit sums fit LDS (BE_ERR_RANGE) — the direct route serves what the layout refuses.
 *   be_scatter_plan_q8_count : fills seg (m * n_slices entries of 8 B), writes order_out (uint16[nnz], or NULL) as
 *       be_scatter_plan_count_ordered does, returns the size of blob in *blob_bytes_host.  SYNCHRONOUS.  scratch >=
 *       be_scatter_plan_q8_scratch_bytes(m, k, slice_shift, slice_width).
 *   caller allocates blob (128-byte aligned, blob_bytes + 128).
 *   be_scatter_plan_q8_fill  : fills blob from codes[nnz]; order = what the count wrote, or NULL (the rows are sorted again).
 *   be_binary_csrm{v,m}_t_plan_f8 : the step.  block_hint, parts and the workspace contract (its first 4 * n_batch bytes ZERO on
 *       entry, zero again after the call) as be_binary_csrmm_t_plan;
 *       workspace >= be_binary_csrmm_t_plan_f8_workspace_bytes(m, k, n_batch, slice_shift, slice_width, parts, block_hint).
 *
 * Gather direction (brainevent_amd/csrc/be_csr_f8_gather.hip): `W8 @ events` over the stored rows, which is `events @ W8.T` of a
 * Float8CSR and `events @ Float8CSC`.  E, Q(c), inv, the "active" rule and the finite-code precondition are those above.  For a
 * matrix of m stored rows over k columns and the spike vector s[k] of batch row b:
 *     R_i       = sum over the stored entries e of row i with s[indices[e]] active, of Q(codes[e])        (int64, exact)
 *     out[b, i] = (float)((double)(long long)R_i * inv)
 * — the finish of the scatter direction, so the gather over a matrix and the scatter over its transpose (the mirror, planned or
 * direct) give the same bits, whatever the lanes-per-row instance.  Spikes: BE_SPIKE_BOOL / FLOAT [n_batch, k], or BE_SPIKE_BITS
 * ([n_batch, ceil(k / 32)] words, read in place); BE_SPIKE_IDS: BE_ERR_UNSUPPORTED.  The workspace holds the packed bitmaps only
 * (be_pack_spikes_batched's layout): no atomics, no accumulators, no convert launch; every out[b, i] is written once.  nnz = the
 * length of codes / indices (no load reaches past it; with an indptr also the lanes-per-row hint); indptr == NULL: rows of
 * row_len entries, and nnz >= m * row_len (BE_ERR_INVALID otherwise).  No alignment is asked of codes or indices beyond their types'.
 * Contracts and the other error conditions as above.
 *   workspace >= be_binary_csrmm_nt_f8_workspace_bytes(m, k, n_batch)
 * ---------------------------------------------------------------------------------------------- */
int64_t be_binary_csrmv_t_f8_workspace_bytes(int64_t m, int64_t k);
int64_t be_binary_csrmm_t_f8_workspace_bytes(int64_t m, int64_t k, int64_t n_batch);
int be_binary_csrmv_t_f8(const void* codes, int f8_format, double scale, const int32_t* indices, const void* indptr,
                         int indptr_is_i64, int64_t row_len, int64_t nnz, const void* spikes, int spike_dtype, void* out_f32,
                         int64_t m, int64_t k, void* workspace, int64_t workspace_bytes, be_stream_t stream);
int be_binary_csrmm_t_f8(const void* codes, int f8_format, double scale, const int32_t* indices, const void* indptr,
                         int indptr_is_i64, int64_t row_len, int64_t nnz, const void* spikes_bm, int spike_dtype, void* out_f32_bm,
                         int64_t m, int64_t k, int64_t n_batch, void* workspace, int64_t workspace_bytes, be_stream_t stream);
int64_t be_binary_csrmv_nt_f8_workspace_bytes(int64_t m, int64_t k);
int64_t be_binary_csrmm_nt_f8_workspace_bytes(int64_t m, int64_t k, int64_t n_batch);
int be_binary_csrmv_nt_f8(const void* codes, int f8_format, double scale, const int32_t* indices, const void* indptr,
                          int indptr_is_i64, int64_t row_len, int64_t nnz, const void* spikes, int spike_dtype, void* out_f32,
                          int64_t m, int64_t k, void* workspace, int64_t workspace_bytes, be_stream_t stream);
int be_binary_csrmm_nt_f8(const void* codes, int f8_format, double scale, const int32_t* indices, const void* indptr,
                          int indptr_is_i64, int64_t row_len, int64_t nnz, const void* spikes_bm, int spike_dtype, void* out_f32_bm,
                          int64_t m, int64_t k, int64_t n_batch, void* workspace, int64_t workspace_bytes, be_stream_t stream);
int64_t be_scatter_plan_q8_scratch_bytes(int64_t m, int64_t k, int slice_shift, int slice_width);
int be_scatter_plan_q8_count(const int32_t* indices, const void* indptr, int indptr_is_i64, int64_t row_len, int64_t m, int64_t k,
                             int slice_shift, int slice_width, void* seg, void* scratch, int64_t scratch_bytes,
                             int64_t* blob_bytes_host, uint16_t* order_out, be_stream_t stream);
int be_scatter_plan_q8_fill(const void* codes, const int32_t* indices, const void* indptr, int indptr_is_i64, int64_t row_len,
                            int64_t m, int64_t k, int slice_shift, int slice_width, const void* seg, void* blob,
                            const uint16_t* order, be_stream_t stream);
int64_t be_binary_csrmv_t_plan_f8_workspace_bytes(int64_t m, int64_t k, int slice_shift, int slice_width, int parts, int block_hint);
int64_t be_binary_csrmm_t_plan_f8_workspace_bytes(int64_t m, int64_t k, int64_t n_batch, int slice_shift, int slice_width, int parts,
                                                  int block_hint);
int be_binary_csrmv_t_plan_f8(const void* blob, const void* seg, int f8_format, double scale, const void* spikes, int spike_dtype,
                              void* out_f32, int64_t m, int64_t k, int slice_shift, int slice_width, int block_hint, int parts,
                              void* workspace, int64_t workspace_bytes, be_stream_t stream);
int be_binary_csrmm_t_plan_f8(const void* blob, const void* seg, int f8_format, double scale, const void* spikes_bm, int spike_dtype,
                              void* out_f32_bm, int64_t m, int64_t k, int64_t n_batch, int slice_shift, int slice_width,
                              int block_hint, int parts, void* workspace, int64_t workspace_bytes, be_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * JIT-connectivity products (the matrix is regenerated on the fly, never stored)
 * replaces: jit_scalar_binary_jitsmv.{pack_bool,notrans_*,trans_*} (brainevent/_jit_scalar/binary_jitsmv.cu:107-321),
 *           jit_scalar_binary_jitsmm.{pack,notrans_*,trans_*} (brainevent/_jit_scalar/binary_jitsmm.cu),
 *           and the uniform / normal twins (brainevent/_jit_uniform/binary_jitumv.cu:77-213, binary_jitumm.cu;
 *           brainevent/_jit_normal/binary_jitnmv.cu:105-312, binary_jitnmm.cu).
 *   mode    : 0 scalar (w = w0), 1 uniform (w = w0 + u01(seed,row,col) * w1, i.e. w0 = low, w1 = high - low),
 *             2 normal (w = w0 + n01(seed,row,col) * w1, i.e. w0 = loc, w1 = scale)
 *   clen    : ceil(2 / prob) as the reference computes it (brainevent/_data.py:1212-1245); values < 2 act as 2;
 *             clen <= 0 (prob = 0) yields zeros
 *   shape1  : shape[1] of the logical matrix — keys the chunk width ceil(shape1 / 4) (brainevent/_misc.py:74-122)
 *   gather  : 1 = "notrans" kernel (corder=True): RNG rows are the out_len outputs, the walk runs over in_len;
 *             0 = "trans" kernel (corder=False): RNG rows are the in_len inputs (only active ones are walked),
 *             the walk runs over out_len
 *   scale_exp : (scatter, modes 1 and 2) fixed-point exponent: edge weights are summed as round(w * 2^scale_exp)
 *             in 64-bit integers; the caller guarantees |w|max * 2^scale_exp * in_len < 2^62
 *   mv walks with lane stride 32, mm with lane stride 4 (a different matrix, as in the reference:
 *   brainevent/_misc.py:32-38)
 * ---------------------------------------------------------------------------------------------- */
/* Armed workspaces of the SCATTER orientation (mv and mm).  A scatter call compacts the spikes through counters at the head of its
 * workspace, which it zeroes first — one more launch per call (4.7 us of a 122-us step at BASELINE config C3).  A workspace that was
 * armed once (its counters zeroed here) skips that launch: the call's last kernel leaves the counters at zero again.  The library
 * keys this on the workspace POINTER: disarm it before the memory is freed or reused for anything else; after a call that returned
 * an error, disarm or arm again.  Results are identical either way.  (The reference compacts per call inside its FFI target and
 * has no workspace to keep: brainevent/_jit_scalar/binary_jitsmv.cu:107-125, :175-214.) */
int be_jit_scatter_workspace_arm(void* workspace, int64_t workspace_bytes, be_stream_t stream);
int be_jit_scatter_workspace_disarm(void* workspace);
int64_t be_binary_jitmv_workspace_bytes(int64_t shape1, int64_t in_len, int64_t out_len, int gather);
int be_binary_jitmv(int mode, double w0, double w1, int wdtype, int64_t clen, uint32_t seed, const void* spikes,
                    int spike_dtype, void* out, int64_t shape1, int64_t in_len, int64_t out_len, int gather,
                    int scale_exp, void* workspace, int64_t workspace_bytes, be_stream_t stream);
/* Multi-GPU partition of the scatter ("trans") orientation with no stored state: the walk of a generator row is a
 * set of independent streams keyed by (chunk, lane) (brainevent/_jit_scalar/binary_jitsmv.cu:54-66), and stream
 * (chunk, lane) only ever touches the output columns chunk_start + lane + stride * q.  A rank that owns the classes
 * [class_begin, class_begin + class_count) (class = chunk * stride + lane; be_jit_scatter_classes() of them in all)
 * therefore owns those columns outright: `out` (full length out_len) receives the owned columns and zeros elsewhere,
 * the outputs of the ranks are disjoint and their sum is the unsharded result.  Workspace: the unsharded query. */
int be_jit_scatter_classes(int64_t shape1, int64_t out_len, int stride);
int be_binary_jitmv_sharded(int mode, double w0, double w1, int wdtype, int64_t clen, uint32_t seed, const void* spikes,
                            int spike_dtype, void* out, int64_t shape1, int64_t in_len, int64_t out_len, int class_begin,
                            int class_count, int scale_exp, void* workspace, int64_t workspace_bytes, be_stream_t stream);
/* ... and of the gather ("notrans") orientation, by OUTPUT ROWS: the generator rows are the outputs there, keyed by (seed, row,
 * chunk, lane) alone, so a rank that owns rows [row_begin, row_begin + row_count) computes exactly those outputs from the full
 * (all-gathered) spike vector — `out` has row_count elements; the ranks' slices concatenate to the unsharded result bit for bit.
 * Workspace: be_binary_jitmv_workspace_bytes(shape1, in_len, row_count, 1). */
int be_binary_jitmv_rows(int mode, double w0, double w1, int wdtype, int64_t clen, uint32_t seed, const void* spikes,
                         int spike_dtype, void* out, int64_t shape1, int64_t in_len, int64_t row_begin, int64_t row_count,
                         void* workspace, int64_t workspace_bytes, be_stream_t stream);
int64_t be_binary_jitmm_workspace_bytes(int64_t shape1, int64_t in_len, int64_t out_len, int64_t n_batch, int gather);
int be_binary_jitmm(int mode, double w0, double w1, int wdtype, int64_t clen, uint32_t seed, const void* spikes_bm,
                    int spike_dtype, void* out_bm, int64_t shape1, int64_t in_len, int64_t out_len, int64_t n_batch,
                    int gather, void* workspace, int64_t workspace_bytes, be_stream_t stream);

/* weights of explicitly listed edges: out[i] = the weight edge (rows[i], cols[i]) carries if the walk generates it —
 * rows / cols in the RNG orientation (the generator row and the walk coordinate).  mode / w0 / w1 as above.  These are the
 * per-edge hashes of the reference, brainevent/_numba_random.py:424-430 (uniform01), :433-486 (normal01), evaluated by
 * the device code the products use; the reference pins them with exact values (brainevent/_numba_random_test.py:58-93). */
int be_jit_edge_weights(int mode, double w0, double w1, uint32_t seed, const int32_t* rows, const int32_t* cols, int64_t n,
                        float* out, be_stream_t stream);

/* materialisation of the generator matrix as CSR (rows = walk owners; stride 32 = the mv matrix, 4 = the mm matrix)
 * replaces: the count + fill kernels of brainevent/_jit_scalar/csr.cu (and the uniform / normal twins).
 *   count: row_counts[n_rows] (uint32) <- number of generated edges per row
 *   fill : caller scans the counts into indptr (int64, n_rows + 1) and allocates indices[nnz] (+ weights[nnz] f32 for
 *          modes 1 / 2); cursor[n_rows] is scratch.  Order inside a row is unspecified. */
int be_jitc_csr_count(int64_t clen, uint32_t seed, int64_t shape1, int64_t n_rows, int64_t walk_len, int stride,
                      uint32_t* row_counts, be_stream_t stream);
int be_jitc_csr_fill(int mode, double w0, double w1, int64_t clen, uint32_t seed, int64_t shape1, int64_t n_rows,
                     int64_t walk_len, int stride, const int64_t* indptr, uint32_t* cursor, int32_t* indices,
                     float* weights, be_stream_t stream);
/* the same rows in canonical order, optionally fused with the per-synapse product (dt2t): for every walk owner r the entries
 * are written in ASCENDING walk coordinate j from indptr[r] on — the column-sorted CSR the reference sorts its
 * materialisation into (brainevent/_jit_scalar/csr.py:562-570) and defines its per-synapse products on
 * (brainevent/_jit_{scalar,uniform,normal}/dt2t.py).  indptr is the scan of be_jitc_csr_count's counts (int64, n_rows + 1).
 *   indices_out[pos] = j                                                      (int32; may be NULL)
 *   values_out[pos]  = w(r, j), times y[r] (y_by_owner) or y[j] when y != NULL  (f32; may be NULL — not both)
 * w is w0 for mode 0 and the per-edge hash otherwise.  No scratch, no global atomics: bitwise the same from call to call. */
int be_jitc_fill_sorted(int mode, double w0, double w1, int64_t clen, uint32_t seed, int64_t shape1, int64_t n_rows,
                        int64_t walk_len, int stride, const int64_t* indptr, const float* y, int y_by_owner,
                        int32_t* indices_out, float* values_out, be_stream_t stream);

/* named per-family / per-dtype symbols: be_binary_jit{s,u,n}{mv,mm}_{notrans,trans}_{f32,f64,f16,bf16} */
#define BE_JIT_MV_ARGS double w0, double w1, int64_t clen, uint32_t seed, const void *spikes, int spike_dtype,    \
                       void *out, int64_t shape1, int64_t in_len, int64_t out_len, int scale_exp,                 \
                       void *workspace, int64_t workspace_bytes, be_stream_t stream
#define BE_JIT_MM_ARGS double w0, double w1, int64_t clen, uint32_t seed, const void *spikes_bm, int spike_dtype, \
                       void *out_bm, int64_t shape1, int64_t in_len, int64_t out_len, int64_t n_batch,            \
                       void *workspace, int64_t workspace_bytes, be_stream_t stream
#define BE_DECL_JIT_FAMILY(F, W)                        \
  int be_binary_jit##F##mv_notrans_##W(BE_JIT_MV_ARGS);  \
  int be_binary_jit##F##mv_trans_##W(BE_JIT_MV_ARGS);    \
  int be_binary_jit##F##mm_notrans_##W(BE_JIT_MM_ARGS);  \
  int be_binary_jit##F##mm_trans_##W(BE_JIT_MM_ARGS);
#define BE_FOR_JIT_VARIANTS(X)                                  \
  X(s, 0, f32, BE_F32) X(s, 0, f64, BE_F64) X(s, 0, f16, BE_F16) X(s, 0, bf16, BE_BF16) \
  X(u, 1, f32, BE_F32) X(u, 1, f64, BE_F64) X(u, 1, f16, BE_F16) X(u, 1, bf16, BE_BF16) \
  X(n, 2, f32, BE_F32) X(n, 2, f64, BE_F64) X(n, 2, f16, BE_F16) X(n, 2, bf16, BE_BF16)
#define BE_DECL_JIT_VARIANT(F, M, W, WD) BE_DECL_JIT_FAMILY(F, W)
BE_FOR_JIT_VARIANTS(BE_DECL_JIT_VARIANT)

/* per-variant symbols (same grammar as the reference's `// @BE` names); thin wrappers of the above */
#define BE_DENSE_MV_ARGS const void *weights, const void *spikes, void *out, int64_t rows_w, int64_t cols_w,      \
                         void *workspace, int64_t workspace_bytes, be_stream_t stream
#define BE_DENSE_MM_ARGS const void *weights, const void *spikes_bm, void *out_bm, int64_t rows_w, int64_t cols_w, \
                         int64_t n_batch, void *workspace, int64_t workspace_bytes, be_stream_t stream
#define BE_CSR_MV_ARGS const void *weights, const int32_t *indices, const void *indptr, int indptr_is_i64,       \
                       const void *spikes, void *out, int64_t m, int64_t k, void *workspace,                      \
                       int64_t workspace_bytes, be_stream_t stream
#define BE_CSR_MM_ARGS const void *weights, const int32_t *indices, const void *indptr, int indptr_is_i64,       \
                       const void *spikes_bm, void *out_bm, int64_t m, int64_t k, int64_t n_batch,                \
                       void *workspace, int64_t workspace_bytes, be_stream_t stream
/* fixed-number connectivity: indices is [n_pre, n_conn] row-major, weights same shape or [1]
 * (brainevent/_fcn/binary_fcnmv.cu:207-251, binary_fcnmm.cu:835-857, 993-1023).
 * scatter: spikes [n_batch, n_pre] -> out [n_batch, n_post];  gather: spikes [n_batch, n_post] -> out [n_batch, n_pre] */
#define BE_FCN_MV_ARGS const void *weights, const int32_t *indices, const void *spikes, void *out,               \
                       int64_t n_pre, int64_t n_post, int64_t n_conn, void *workspace, int64_t workspace_bytes,   \
                       be_stream_t stream
#define BE_FCN_MM_ARGS const void *weights, const int32_t *indices, const void *spikes_bm, void *out_bm,         \
                       int64_t n_pre, int64_t n_post, int64_t n_conn, int64_t n_batch, void *workspace,           \
                       int64_t workspace_bytes, be_stream_t stream

#define BE_DECL_VARIANT(W, WD, S, SD)                            \
  int be_binary_csrmv_t_homo_##W##_##S(BE_CSR_MV_ARGS);           \
  int be_binary_csrmv_t_hetero_##W##_##S(BE_CSR_MV_ARGS);         \
  int be_binary_csrmv_nt_homo_##W##_##S(BE_CSR_MV_ARGS);          \
  int be_binary_csrmv_nt_hetero_##W##_##S(BE_CSR_MV_ARGS);        \
  int be_binary_csrmm_t_homo_##W##_##S(BE_CSR_MM_ARGS);           \
  int be_binary_csrmm_t_hetero_##W##_##S(BE_CSR_MM_ARGS);         \
  int be_binary_csrmm_nt_homo_##W##_##S(BE_CSR_MM_ARGS);          \
  int be_binary_csrmm_nt_hetero_##W##_##S(BE_CSR_MM_ARGS);        \
  int be_binary_fcnmv_scatter_homo_##W##_##S(BE_FCN_MV_ARGS);     \
  int be_binary_fcnmv_scatter_hetero_##W##_##S(BE_FCN_MV_ARGS);   \
  int be_binary_fcnmv_gather_homo_##W##_##S(BE_FCN_MV_ARGS);      \
  int be_binary_fcnmv_gather_hetero_##W##_##S(BE_FCN_MV_ARGS);    \
  int be_binary_fcnmm_scatter_homo_##W##_##S(BE_FCN_MM_ARGS);     \
  int be_binary_fcnmm_scatter_hetero_##W##_##S(BE_FCN_MM_ARGS);   \
  int be_binary_fcnmm_gather_homo_##W##_##S(BE_FCN_MM_ARGS);      \
  int be_binary_fcnmm_gather_hetero_##W##_##S(BE_FCN_MM_ARGS);    \
  int be_binary_densemv_transpose_##W##_##S(BE_DENSE_MV_ARGS);    \
  int be_binary_densemv_no_transpose_##W##_##S(BE_DENSE_MV_ARGS); \
  int be_binary_densemm_transpose_##W##_##S(BE_DENSE_MM_ARGS);    \
  int be_binary_densemm_no_transpose_##W##_##S(BE_DENSE_MM_ARGS);

/* ------------------------------------------------------------------------------------------------
 * Spike-triggered plasticity (pair-based additive STDP).  Replaces the reference's update primitives:
 *   update_csr_on_binary_pre  (brainevent/_csr/plasticity_binary.py:45-173, kernel plasticity_binary_on_pre.cu)
 *   update_csr_on_binary_post (brainevent/_csr/plasticity_binary.py:477-618: CSC arrays + the CSC->CSR permutation)
 *   update_csc_on_binary_pre / _post (brainevent/_csr/plasticity_binary.py:968-1160: the same two with the roles swapped)
 *   update_fixed_post_conn_on_binary_pre / update_fixed_pre_conn_on_binary_post (brainevent/_fcn/plasticity_binary.py:207-300)
 *   update_dense_on_binary_pre / _post (brainevent/_dense/plasticity_binary.py:42-140, :360-458)
 * Rule: for every active row r (spike != 0; float spikes: any nonzero value) and every stored slot k of r:
 *   w[perm ? perm[k] : k] = w[...] + trace[indices[k]]      one rounding to the weight dtype (f16 / bf16 add in f32);
 * then, when clip_lo / clip_hi is set, min(max(w, w_lo), w_hi) on the TOUCHED entries (NaN stays NaN; w_lo > w_hi gives
 * w_hi).  The reference clips the whole array: a caller that cannot certify the untouched entries calls with no bound and
 * clamps the whole array itself.  trace has the weight dtype; w_lo / w_hi are values of the weight dtype.
 * Row-driven (perm = NULL): CSR pre, CSC post, FixedNumPerPre pre / FixedNumPerPost post (indptr = NULL, row_len = num_conn).
 * Permuted (perm = int32 / int64 map of the transposed structure's slots to weight positions, each position listed once):
 * CSR post, CSC pre, FixedNumPerPre post, FixedNumPerPost pre, with indptr / indices = the transposed structure.
 * spike_dtype: BE_SPIKE_BOOL, BE_SPIKE_FLOAT, BE_SPIKE_BITS, BE_SPIKE_IDS.  nnz = number of slots (sizes the grid).
 * No atomics: every weight is written by one lane.  The host is never synchronised (graph-capturable).
 * ---------------------------------------------------------------------------------------------- */
int64_t be_plasticity_workspace_bytes(int64_t n_rows);
int be_plasticity_rows(void* weights, int wdtype, const int32_t* indices, const void* indptr, int indptr_is_i64,
                       int64_t row_len, int64_t nnz, const void* perm, int perm_is_i64, const void* spikes, int spike_dtype,
                       int64_t n_rows, const void* trace, int clip_lo, double w_lo, int clip_hi, double w_hi,
                       void* workspace, int64_t workspace_bytes, be_stream_t stream);
/* The permuted walk with an AGED trace: the post-spike update of delayed synapses (brainevent_amd/_delay.py).
 * t_indptr [n_post + 1] / t_rows / perm are the transposed structure of a matrix STACKED by delay (stacked row d * n_pre + i =
 * the entries of row i with delay d, d < ages); values[ring_depth][n_pre] (the weight dtype) and head[1] are a value ring
 * (be_value_ring_push): for slot k of every active post neuron, with r = t_rows[k], d = r / n_pre, i = r - d * n_pre,
 *   w[perm[k]] = w[perm[k]] + values[((*head - 1 - d) mod ring_depth) * n_pre + i]
 * with the rounding, the clip, the spike encodings and the workspace of be_plasticity_rows (n_rows = n_post).  perm is required;
 * ages <= ring_depth, ring_depth * n_pre < 2^31.  *head is read on the device: graph-capturable. */
int be_plasticity_rows_aged(void* weights, int wdtype, const int32_t* t_rows, const void* t_indptr, int indptr_is_i64,
                            int64_t nnz, const void* perm, int perm_is_i64, const void* spikes, int spike_dtype,
                            int64_t n_post, const void* values, const int32_t* head, int64_t n_pre, int ring_depth, int ages,
                            int clip_lo, double w_lo, int clip_hi, double w_hi, void* workspace, int64_t workspace_bytes,
                            be_stream_t stream);
/* Dense row-major weights [n_rows, n_cols].  pre = 1: spikes [n_rows], trace [n_cols], active row i gets += trace.
 * pre = 0: spikes [n_cols], trace [n_rows], w[i, j] += trace[i] for each active column j.  Workspace: n = n_rows (pre)
 * or n_cols (post). */
int be_plasticity_dense(int pre, void* weights, int wdtype, int64_t n_rows, int64_t n_cols, const void* spikes,
                        int spike_dtype, const void* trace, int clip_lo, double w_lo, int clip_hi, double w_hi,
                        void* workspace, int64_t workspace_bytes, be_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Weight gradients of the event-driven products (the backward pass of brainevent_amd/_autograd.py).  The reference's
 * derivative rules: brainevent/_csr/binary.py:656-715 (mv), :1303-1360 (mm, SDDMM), brainevent/_dense/binary.py:290-330,
 * brainevent/_fcn/binary.py:317-.  a = active(spike) (the forward kernels' rule: != 0 for bytes, > 0 for f32), g = the
 * incoming gradient of the output, r(j) / c(j) = row / column of stored entry j:
 *   transpose = 1 (s @ A):  dw[j] = sum_b a[b, r(j)] * g[b, c(j)]      transpose = 0 (A @ s):  dw[j] = sum_b g[b, r(j)] * a[b, c(j)]
 *   homo = 1: the scalar sum over j of the same (dw has one element).
 * Sums run over the active b only, in ascending b, in f32 (f64 for f64 weights), rounded once to the weight dtype.  Every
 * entry is written once (zeros for an inactive row, without reading its indices); no atomics; the homogeneous sum is a
 * fixed-order two-pass reduction (deterministic).  Never synchronises the host (graph-capturable).
 *
 * be_grad_pack_activity: the activity of a batch-major spike buffer [n_batch, n] (BE_SPIKE_BOOL / BE_SPIKE_FLOAT; BE_SPIKE_BITS:
 * [n_batch, ceil(n/32)] words; BE_SPIKE_IDS: one vector) as the per-neuron bit mask mask[n][ceil(n_batch/32)] (bit b % 32 of
 * word b / 32), be_grad_mask_bytes(n, n_batch) bytes.
 * be_grad_pack_activity_aged (csrc/be_neuron_sg_rec_delay.hip; ONE launch): the activity of the stacked rows of a delay split over
 * the T * B batch rows (t, b) of be_lif_rec_delay_sg_backward's g_x, from the layer's f32 spikes s [T, B, N] and s_hist
 * [hist_ages, B, N] (active where != 0): mask[depth * N][ceil(T * B / 32)], bit p % 32 of word p / 32 of row d * N + i, p = t * B + b,
 * = sp(t - 1 - d)[b][i] — neuron i's spike train shifted by d steps, history included, silence before it;
 * be_grad_mask_bytes(depth * N, T * B) bytes, every word written.  BE_ERR_INVALID: B < 1, T < 1, T * B > 65535, depth outside
 * 1 .. 256, hist_ages outside 0 .. depth, a NULL pointer that is needed.
 * be_grad_rows: CSR rows (indptr int32 / int64) or fixed-length rows (indptr = NULL, row_len = num_conn, nse = n_rows *
 * row_len).  mask has one row per stored row (transpose = 1) or per column id (transpose = 0).  g is the weight dtype; its
 * element (batch b, neuron x) is g[x * g_sn + b * g_sb], x a column id (transpose = 1) or a row (transpose = 0).
 * be_grad_dense: W [n_rows, n_cols] row-major.  transpose = 1 (events @ W): dW[i, j] = sum_{b: a[b, i]} g(b, j), mask over
 * the rows; transpose = 0 (W @ events): dW[i, j] = sum_{b: a[b, j]} g(b, i), mask over the columns.
 * ---------------------------------------------------------------------------------------------- */
int64_t be_grad_mask_bytes(int64_t n, int64_t n_batch);
int be_grad_pack_activity(const void* spikes, int spike_dtype, int64_t n, int64_t n_batch, uint32_t* mask, be_stream_t stream);
int be_grad_pack_activity_aged(const float* s, const float* s_hist, int64_t N, int64_t B, int64_t T, int depth, int hist_ages,
                               uint32_t* mask, be_stream_t stream);
int64_t be_grad_rows_workspace_bytes(int64_t nse);
int be_grad_rows(int transpose, void* dw, int homo, int wdtype, const int32_t* indices, const void* indptr, int indptr_is_i64,
                 int64_t row_len, int64_t n_rows, int64_t nse, const uint32_t* mask, int64_t n_batch, const void* g,
                 int64_t g_sn, int64_t g_sb, void* workspace, int64_t workspace_bytes, be_stream_t stream);
int64_t be_grad_dense_workspace_bytes(int64_t n_rows, int64_t n_cols);
int be_grad_dense(int transpose, void* dw, int wdtype, int64_t n_rows, int64_t n_cols, const uint32_t* mask, int64_t n_batch,
                  const void* g, int64_t g_sn, int64_t g_sb, be_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * the sampled dense-dense product on a stored pattern (SDDMM): one value per stored entry e of row r(e) and stored index c(e),
 *   out[e] = sum_{b < n_batch} p[r(e) * n_batch + b] * q[c(e) * n_batch + b]
 * replaces: sddmm_indices / sddmm_coo_indices (brainevent/_sddmm.py) and the mm weight rule of the float-operand products
 *           (brainevent/_csr/float.py:825-860; mv, :287-330, is n_batch = 1): A @ X -> p = g, q = X; A.T @ X -> p = X, q = g.
 * p [n_rows, n_batch], q [n_cols, n_batch] and out [nse] are in the weight dtype (f32 / f64 / f16 / bf16), p and q contiguous.
 * The row of an entry comes from row_ids [nse] when it is not NULL (COO), else from indptr (int32 / int64, n_rows + 1 entries
 * ascending from 0 to nse; empty rows allowed), else from the fixed row length row_len > 0 (r = e / row_len).  An entry whose
 * row or stored index lies outside [0, n_rows) / [0, n_cols) gets 0; nothing is read through it.
 * Sums run in f32 (f64 for f64) and are rounded once.  The lanes that share an entry, and with them the order of its sum,
 * depend on n_batch and the dtype only — not on the grid, the row lengths, the row source or the alignment of p and q (which
 * only picks 16-byte or element loads) — so results are bit-identical across runs and across the three row sources.  Every
 * entry is written exactly once: no memset, no atomics, no workspace, no host synchronisation (graph-capturable).  Work is
 * balanced per entry; entry offsets are 64-bit.  nse = 0, n_batch = 0 or n_rows = 0 returns without a launch.
 * ---------------------------------------------------------------------------------------------- */
int be_sddmm_rows(void* out, int wdtype, const int32_t* indices, const void* indptr, int indptr_is_i64, int64_t row_len,
                  const int32_t* row_ids, int64_t n_rows, int64_t n_cols, int64_t nse, const void* p, const void* q,
                  int64_t n_batch, be_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * container arithmetic on a stored pattern (csrc/be_arith.hip).
 *
 * be_entries_dense_op: a dense operand sampled on the pattern, one value per stored entry e of row r(e), stored index c(e):
 *   out[e] = op(weights[w_homo ? 0 : e], dense[r(e) * stride_row + c(e) * stride_col]),  op: 0 take (the dense value alone;
 *   weights may be NULL), 1 mul (w * d), 2 div (w / d), 3 rdiv (d / w).
 * replaces: the dense-operand branch of the binary operators (brainevent/_csr/main.py:1532-1543, :1580-1591 and the fixed-number
 *           twins), without the row id array of nse integers.
 * weights and out [nse] are in the weight dtype (f32 / f64 / f16 / bf16); dense is read in place through its two int64 ELEMENT
 * strides, in the weight dtype or (dense_is_u8) as bytes holding a number (a bool / uint8 mask).  The row of an entry comes
 * from indptr (int32 / int64, n_rows + 1 entries ascending from 0 to nse; empty rows allowed), else from the fixed row length
 * row_len > 0.  An entry whose row or stored index lies outside [0, n_rows) / [0, n_cols) uses 0 for the dense value; nothing
 * is read through it.  One operation in f32 (f64 for f64) and one rounding.  Every entry is written exactly once: no memset,
 * no atomics, no workspace, no host synchronisation (graph-capturable).  Work is balanced per entry; entry offsets are 64-bit.
 *
 * be_diag_scan / be_diag_move / be_diag_fill: A + diag(d) on CSR arrays with the missing diagonal entries inserted
 * replaces: csr_diag_position / csr_diag_add (brainevent/_csr/diag_add.py), on the device and past 2^31 entries.
 *   scan: found [n_diag, 2] int64, set by the caller to (-1, INT64_MAX) per row: [r][0] <- the largest entry offset of row r
 *         with index == r, [r][1] <- the smallest with index > r (64-bit integer atomic max / min: order-independent).
 *   move: entry e of row r goes to dst = e + shift[r] + (0 <= ins[r] <= e): new_indices[dst] = indices[e], new_data[dst] =
 *         weights[w_homo ? 0 : e], old_to_new[e] = dst (int32 / int64) — each of the three only where its pointer is not NULL.
 *   fill: per i < n_diag, dest = (exist[i] >= 0 ? exist[i] : ins[i]) + shift[i]: new_indices[dest] = i where exist[i] < 0,
 *         new_data[dest] = (exist[i] >= 0 ? weights[exist[i]] : 0) + diag[i], one addition in f32 (f64) and one rounding.
 *         Launch it after move on the same stream: an existing diagonal is written by both, fill last.
 * shift / ins [n_rows] and exist [n_diag] are int64 (the per-row plan brainevent_amd/_diag.py derives from `found`); a
 * destination outside [0, new_nse) is skipped.  No memset, no float atomics, no host synchronisation.
 * ---------------------------------------------------------------------------------------------- */
int be_entries_dense_op(void* out, const void* weights, int w_homo, int wdtype, const int32_t* indices, const void* indptr,
                        int indptr_is_i64, int64_t row_len, int64_t n_rows, int64_t n_cols, int64_t nse, const void* dense,
                        int dense_is_u8, int64_t stride_row, int64_t stride_col, int op, be_stream_t stream);
int be_diag_scan(const int32_t* indices, const void* indptr, int indptr_is_i64, int64_t n_rows, int64_t n_diag, int64_t nse,
                 void* found, be_stream_t stream);
int be_diag_move(const void* weights, int w_homo, int wdtype, const int32_t* indices, const void* indptr, int indptr_is_i64,
                 int64_t n_rows, int64_t nse, const int64_t* shift, const int64_t* ins, int64_t new_nse, int32_t* new_indices,
                 void* new_data, void* old_to_new, int old_to_new_is_i64, be_stream_t stream);
int be_diag_fill(const void* weights, int w_homo, int wdtype, int64_t nse, int64_t n_diag, const int64_t* shift,
                 const int64_t* ins, const int64_t* exist, const void* diag, int64_t new_nse, int32_t* new_indices,
                 void* new_data, be_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * A x = b on CSR arrays (csrc/be_solve.hip): right-preconditioned BiCGSTAB with the Jacobi preconditioner D^-1 (D_ii = the sum
 * of the stored (i, i) entries, 1 where that sum is zero or the diagonal is absent).
 * replaces: CSR.solve / csr_solve (brainevent/_csr/main.py:1778-1814, _csr/spsolve.py: cuSOLVER sparse QR) — the method here is
 *           ITERATIVE; brainevent_amd/_solve.py drives it and states its contract.
 * The matrix is n x n with n < 2^31, weights f32 / f64 (per entry, nnz of them), indices int32, indptr int32 / int64 (n + 1
 * entries ascending from 0 to nnz); entries of a row in any order, duplicates add.  weights, indices and x are 16-byte aligned;
 * b, x and the work vectors are in the weight dtype.  One workspace of be_solve_workspace_bytes(n, wdtype) bytes holds the state
 * (first 72 bytes: doubles rho, rho_old, alpha, omega, rr; int32 status (0 running, 1 converged, 2 breakdown), iterations,
 * first, offdiag, n_rr, half), the partial sums, seven work vectors and D^-1; the same workspace goes to every call of one solve.
 *   setup:    zeroes the state, writes D^-1 (and D, for `diagonal`); offdiag <- 1 when a nonzero entry lies off the diagonal.
 *   residual: r = b - A x (x = NULL: r = b, the matrix is not read), rh = r, rr <- |r|^2, status, half <- 0, first <- 1: the start,
 *             a restart with residual replacement, and the TRUE residual of a result.  Two launches.
 *   diagonal: x = b / D, one rounding per element (for a matrix with offdiag = 0).
 *   iterate:  n_iter (1..64) iterations of five launches each and one single-workgroup launch that leaves rr and status for the
 *             host.  |r|^2 <= thr2 sets status 1, a vanishing or non-finite rho, rh.v, t.t or omega sets status 2; |s|^2 <= thr2
 *             at the half step sets `half` (every workgroup of that launch still applies x += alpha y; the next launch turns
 *             `half` into status 1, so the host reads status alone); from then on every kernel of the chunk returns at once.
 *             iterations counts the iterations done.
 * Dot products accumulate in f64 and are reduced in a fixed order over grids that depend on (n, nnz) alone; no float atomics,
 * no cooperative launch, no host synchronisation (the caller reads the state back between chunks): bit-identical results
 * from call to call.  Offsets are 64-bit.
 * ---------------------------------------------------------------------------------------------- */
int64_t be_solve_workspace_bytes(int64_t n, int wdtype);
int be_solve_setup(const void* weights, int wdtype, const int32_t* indices, const void* indptr, int indptr_is_i64, int64_t n,
                   int64_t nnz, void* workspace, int64_t workspace_bytes, be_stream_t stream);
int be_solve_residual(const void* weights, int wdtype, const int32_t* indices, const void* indptr, int indptr_is_i64, int64_t n,
                      int64_t nnz, const void* b, const void* x, void* workspace, int64_t workspace_bytes, be_stream_t stream);
int be_solve_diagonal(int wdtype, int64_t n, const void* b, void* x, void* workspace, int64_t workspace_bytes,
                      be_stream_t stream);
int be_solve_iterate(const void* weights, int wdtype, const int32_t* indices, const void* indptr, int indptr_is_i64, int64_t n,
                     int64_t nnz, void* x, int n_iter, double thr2, void* workspace, int64_t workspace_bytes, be_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * synaptic delays on the presynaptic side (brainevent_amd/csrc/be_delay.hip; the reference has no delays)
 *
 * Delay split: the stored rows (indptr, or indptr = NULL and rows of row_len entries) of an m-row matrix and one delay in
 * [0, depth) per stored entry become the STACKED matrix of depth * m rows: stacked row d * m + i holds the entries of row i whose
 * delay is d, in their original relative order (stable).  1 <= depth <= 256.
 *   be_delay_split_count: counts[0] = 0, counts[1 + d * m + i] = entries of row i with delay d (counts: depth * m + 1 elements, int64
 *     when out_is64, else int32); the inclusive scan of counts is indptr_s (the caller scans).  workspace[0..8): the smallest
 *     position whose delay lies outside [0, depth), as int64; -1 when there is none (rewritten by every call).  Such an entry is
 *     skipped by both passes and indexes nothing.
 *   be_delay_split_fill: perm[p] = original position of stacked position p (the element type of indptr_s: out_is64),
 *     indices_s[p] = indices[perm[p]] (optional: NULL), row_mask[d * ceil(m/32) + i/32] bit i%32 = stacked row d * m + i is not
 *     empty (optional: NULL).  No entry-sized temporary, no row-id array, no global atomic places an entry.
 * Neither call synchronises the host.
 *
 * Spike ring: bits[depth][ceil(n/32)] uint32 words (bit i%32 of word i/32, the BE_SPIKE_BITS layout per slot), head[1] and
 * arrivals[1], all on the device and zero to begin with.  depth * n < 2^31.
 *   be_spike_ring_push: packs spikes[n] (BE_SPIKE_BOOL, BE_SPIKE_FLOAT, or BE_SPIKE_BITS words, whose bits past n are dropped) into
 *     slot *head, then *head = (*head + 1) % depth — one launch, no host read; arrivals is the launch's own ticket word and is zero
 *     again when it ends.  The spikes of age a (0: the last push) lie in slot (*head - 1 - a) mod depth.
 *   be_spike_ring_compact: for a in [0, ages), ages <= depth, and every bit i set in the slot of age a AND in row_mask[a] (word
 *     for word; row_mask = NULL keeps all), a * n + i is appended to active_ids (room for ages * n), in no particular order, each
 *     once; *count = how many.  *count is zeroed on the stream by the call itself.  {active_ids, count} is a be_spike_ids_t over
 *     ages * n positions: the BE_SPIKE_IDS operand of the scatter entry points for the stacked matrix.
 * Both are graph-capturable: head is read on the device.
 *
 * Batched spike ring: n_batch histories under ONE head — bits[depth][n_batch][ceil(n/32)], head[1] and
 * arrivals[1] as above; 1 <= n_batch <= 65535 (the batch row is the second grid dimension of both kernels, not strided over).
 *   be_spike_ring_push_batch: be_spike_ring_push for batch-major spikes[n_batch][n] (BE_SPIKE_BITS: [n_batch][ceil(n/32)] words,
 *     bits past n of every row dropped): row b goes to bits[*head][b][.], then *head advances once.  One launch over the grid (bit
 *     tiles, batch rows); every workgroup reads head before it takes its ticket, the last of all tickets advances it.
 *     n_batch = 1 is be_spike_ring_push.
 *   be_spike_ring_unroll: the histories by age as the bit-packed batch operand of the stacked matrix (BE_SPIKE_BITS rows over
 *     ages * n positions): for a < ages <= depth and i < n, with p = a * n + i, bit p % 32 of word p / 32 of out row b (rows of
 *     ceil(ages * n / 32) words) = bit i of slot (*head - 1 - a) mod depth of sample b, ANDed with bit i of row_mask[a] (rows of
 *     ceil(n/32) words; NULL keeps all); the bits from ages * n to the end of a row's last word are 0.  ages * n < 2^31.  Every
 *     output word is written exactly once, by a vector store: no atomics, nothing is zeroed beforehand, no memset node.
 * Both are graph-capturable and synchronise nothing.
 *
 * Value ring: values[depth][n] in one of the four float dtypes (wdtype), head[1] and arrivals[1] as above, zero to begin with.
 *   be_value_ring_push: writes x[n] (x_dtype: any of the four; converted as a cast does, f64 -> f16 / bf16 through f32) into slot
 *     *head, then *head = (*head + 1) % depth — one launch, no host read, arrivals as above.  The vector of age a lies in slot
 *     (*head - 1 - a) mod depth: what be_plasticity_rows_aged reads.
 * ---------------------------------------------------------------------------------------------- */
int64_t be_delay_split_workspace_bytes(int64_t m, int depth);
int be_delay_split_count(const void* indptr, int indptr_is_i64, int64_t row_len, const int32_t* delays, int64_t m, int depth,
                         void* counts, int out_is_i64, void* workspace, int64_t workspace_bytes, be_stream_t stream);
int be_delay_split_fill(const void* indptr, int indptr_is_i64, int64_t row_len, const int32_t* delays, const int32_t* indices,
                        int64_t m, int depth, const void* indptr_s, int out_is_i64, void* perm, int32_t* indices_s,
                        uint32_t* row_mask, be_stream_t stream);
int be_spike_ring_push(const void* spikes, int spike_dtype, int64_t n, int depth, uint32_t* bits, int32_t* head,
                       uint32_t* arrivals, be_stream_t stream);
int be_spike_ring_compact(const uint32_t* bits, const int32_t* head, int64_t n, int depth, int ages, const uint32_t* row_mask,
                          uint32_t* active_ids, uint32_t* count, be_stream_t stream);
int be_value_ring_push(const void* x, int x_dtype, int64_t n, int depth, void* values, int wdtype, int32_t* head,
                       uint32_t* arrivals, be_stream_t stream);
int be_spike_ring_push_batch(const void* spikes, int spike_dtype, int64_t n, int depth, int64_t n_batch, uint32_t* bits,
                             int32_t* head, uint32_t* arrivals, be_stream_t stream);
int be_spike_ring_unroll(const uint32_t* bits, const int32_t* head, int64_t n, int depth, int64_t n_batch, int ages,
                         const uint32_t* row_mask /* [>= ages][ceil(n/32)] or NULL */,
                         uint32_t* out /* [n_batch][ceil(ages*n/32)] */, be_stream_t stream);

#define BE_FOR_ALL_VARIANTS(X) \
  X(f32, BE_F32, bool, BE_SPIKE_BOOL)   X(f32, BE_F32, float, BE_SPIKE_FLOAT)   \
  X(f64, BE_F64, bool, BE_SPIKE_BOOL)   X(f64, BE_F64, float, BE_SPIKE_FLOAT)   \
  X(f16, BE_F16, bool, BE_SPIKE_BOOL)   X(f16, BE_F16, float, BE_SPIKE_FLOAT)   \
  X(bf16, BE_BF16, bool, BE_SPIKE_BOOL) X(bf16, BE_BF16, float, BE_SPIKE_FLOAT)

BE_FOR_ALL_VARIANTS(BE_DECL_VARIANT)

/* ------------------------------------------------------------------------------------------------
 * be_jit_param_grad: the parameter gradients of a JIT-connectivity product (brainevent_amd/csrc/be_jitc_grad.hip)
 * replaces: the reference's per-parameter composition — a whole float product with the parameters set to (1, 0) / (0, 1) and a
 *           dot product each (brainevent/_jit_normal/binary.py:442-505, _jit_normal/float.py:843-910 and the scalar / uniform twins).
 * The generator of (shape1, n_rows, walk_len, stride, clen, seed) — rows = walk owners, as be_jitmm_float walks it — carries
 * w = w0 + t(r, j) * w1 on edge (r, j) (t: the uniform / normal hash of the family `mode`; scalar: w = w0).  With P [n_rows, nb]
 * and Q [walk_len, nb], contiguous, both of `wdtype`:
 *   sums[0] = S0 = sum_edges sum_b P[r, b] Q[j, b]        sums[1] = S1 = sum_edges t(r, j) sum_b P[r, b] Q[j, b]    (scalar: 0)
 * One walk whatever nb is; loads are widened to f64, products and sums are f64, t is the f32 value the products use.  A
 * generator row whose P row is all zero is not walked.  No float atomics: fixed shuffle trees and fixed orders over a grid that
 * depends on (shape1, n_rows, walk_len, stride) alone, so the 16 bytes are the same from call to call.  clen <= 0, n_rows == 0,
 * walk_len == 0 or nb == 0: two zeros are written on the stream and nothing is read.  n_rows, walk_len < 2^32; 64-bit offsets.
 * No host synchronisation (graph-capturable).
 * ---------------------------------------------------------------------------------------------- */
int64_t be_jit_param_grad_workspace_bytes(int64_t shape1, int64_t n_rows, int64_t walk_len, int stride);
int be_jit_param_grad(int mode, int wdtype, int64_t clen, uint32_t seed, const void* P, const void* Q, int64_t shape1,
                      int64_t n_rows, int64_t walk_len, int64_t nb, int stride, double* sums /* [2]: S0, S1 */,
                      void* workspace, int64_t workspace_bytes, be_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* BRAINEVENT_AMD_H */
