"""brainevent_amd — MI355X-native event-driven sparse matmul (brainevent-compatible ``@`` surface).

Only the spike-triggered SpMV/SpMM hot path of chaobrain/brainevent is provided:
``BinaryArray @ {CSR, CSC, dense, JITC{Scalar,Normal,Uniform}{R,C}, FixedNumPerPre/PerPost}`` and the
functional ``binary_*`` operators, running hand-written HIP kernels (gfx950) through a C ABI, and the spike-triggered
plasticity updates (``update_*_on_binary_pre/post``, ``update_on_pre`` / ``update_on_post``).  The products are
differentiable under ``torch.autograd`` (weights and float spikes; ``brainevent_amd._autograd``), and so are the float-operand
products of the same containers (``csr @ x``); ``sddmm_*`` / ``M.sddmm`` sample a dense-dense product on a sparsity pattern.
The JIT-connectivity products are differentiable in their parameters (``weight``; ``w_low, w_high``; ``w_loc, w_scale``) and
their operand: both parameter gradients of a call come out of one walk of the generated edges (``jit_param_sums``).
``CSR.solve`` / ``CSC.solve`` / ``csr_solve`` solve ``A x = b`` by Jacobi-preconditioned BiCGSTAB on the device (``_solve``).
``SpikeRing @ DelayedCSR`` gives every synapse a conduction delay: a bit-packed spike history and the matrix split by delay, one
ordinary scatter per step (``_delay``).  Delayed synapses learn: ``DelayedCSR.update_on_pre`` / ``update_on_post`` (the pre-side
value of a synapse comes from a ``ValueRing``, read by age), and ``ring @ D`` is differentiable in the weights.
The dense products also take OCP FP8 weights (``float8_e4m3fn`` / ``float8_e5m2`` tensors, ``Float8Dense``, ``quantize_fp8``;
``_dense_f8``): a byte per weight, f32 sums, f32 out.  So does the CSR scatter: ``Float8CSR`` / ``CSR.quantize_fp8`` (``_csr_f8``),
two bytes per synapse in its plan, exact 64-bit integer sums, f32 out; ``W8.T`` / ``Float8CSC`` is the other view of the same
arrays and gives the gather direction (a streaming kernel, or the mirror once ``build_mirror()`` was asked for), same bits.
``lif_step`` / ``lif_sequence`` are the spiking neuron between two products, with its surrogate gradient: one launch forwards and
one backwards for a step or a whole input sequence (``_neuron_sg``); ``synaptic_lif_step`` / ``synaptic_lif_sequence`` are the same
with a synaptic current in front of the membrane and an optional adaptive threshold, ``parametric_synaptic_lif_step`` /
``parametric_synaptic_lif_sequence`` that neuron with learnable, per-neuron parameters (``_neuron_syn_sg``); ``recurrent_lif_sequence``
runs that neuron with a sparse recurrent projection inside the time loop, a whole sequence per launch, and
``parametric_recurrent_lif_sequence`` that layer with learnable, per-neuron parameters (``_neuron_rec_sg``); given a ``DelayedCSR``
as the recurrence, ``recurrent_lif_sequence`` runs the layer with a conduction delay per synapse — a sample's spike history stays on
the chip —, still one launch each way and differentiable through the spikes, the history and ``stacked.data``.
"""
from ._version import __version__
__version_info__ = tuple(int(p) for p in __version__.split('.')[:3] if p.isdigit())
from ._error import (BrainEventError, MathError, KernelError, KernelNotAvailableError, KernelCompilationError,
                     KernelFallbackExhaustedError, KernelExecutionError, KernelLoadError, UnsupportedOperationError,
                     BenchmarkDataFnNotProvidedError, KernelToolchainError, CompilationError, KernelRegistrationError)
from . import config
from ._registry import get_registry, get_primitives_by_tags, get_all_primitive_names
from ._event import EventRepresentation, BinaryArray, BitPackedBinary, CompactBinary, bitpack
from ._csr import (CSR, CSC, ScatterPlan, BinnedScatter, check_binned_status, PlannedMatrix, Mirror, indexed_workspace, build_mirror_of, hybrid_task_capacity, binary_csrmv, binary_csrmm, binary_csrmv_indexed, binary_csrmm_indexed, binary_csrmv_indexed_p, binary_csrmm_indexed_p, binary_csrmv_p, binary_csrmm_p,
                   binary_csrmv_p_call, binary_csrmm_p_call)
from ._fcn import (FixedNumConn, FixedNumPerPre, FixedNumPerPost, binary_fcnmv, binary_fcnmm, binary_fcnmv_p,
                   binary_fcnmm_p, binary_fcnmv_p_call, binary_fcnmm_p_call)
from ._dense import (Dense, binary_densemv, binary_densemm, binary_densemv_p, binary_densemm_p, binary_densemv_p_call,
                     binary_densemm_p_call)
from ._dense_f8 import Float8Dense, quantize_fp8
from ._csr_f8 import Float8CSR, Float8CSC, Q8Plan
from ._convert import (csr_to_coo_index, coo_to_csc_index, coo2csr, csr_to_csc_index, csc_to_csr_index,
                       fixed_conn_num_csr_indptr, fixed_conn_num_csc_structure, fixed_conn_num_to_csc, CscBuilder)
from ._float import (csrmv, csrmm, csrmv_p, csrmm_p, csrmv_p_call, csrmm_p_call, fcnmv, fcnmm, fcnmv_p, fcnmm_p, fcnmv_p_call,
                     fcnmm_p_call)
from ._dt2t import (csrmv_dt2t, csrmm_dt2t, cscmv_dt2t, cscmm_dt2t, fcnmv_dt2t, fcnmm_dt2t, csrmv_dt2t_p, csrmm_dt2t_p,
                    fcnmv_dt2t_p, fcnmm_dt2t_p, csrmv_dt2t_p_call, csrmm_dt2t_p_call, fcnmv_dt2t_p_call, fcnmm_dt2t_p_call)
from ._sddmm import sddmm_indices, sddmm_coo_indices, sddmm_p, sddmm_p_call
from ._slice import (csr_slice_rows, csr_slice_rows_p, csr_slice_rows_p_call, csr_slice_rows_grad, csr_slice_rows_grad_p,
                     csr_slice_rows_grad_p_call)
from ._arith import ArithmeticMixin, entries_dense_op_p
from ._diag import csr_diag_position, csr_diag_add
from ._solve import csr_solve, csr_solve_p, csr_solve_p_call
from ._delay import SpikeRing, ValueRing, DelayedCSR
from ._graph import GraphedStep, capture_step
from ._tuning import (ScatterTuning, DEFAULT_SCATTER_TUNING, get_scatter_tuning, save_scatter_tuning, apply_scatter_tuning,
                      tune_scatter_routes)
from ._neuron import lif_coba_step, lif_cuba_step
from ._neuron_sg import lif_step, lif_sequence
from ._neuron_syn_sg import (synaptic_lif_step, synaptic_lif_sequence, parametric_synaptic_lif_step,
                             parametric_synaptic_lif_sequence)
from ._neuron_rec_sg import recurrent_lif_sequence, parametric_recurrent_lif_sequence
from ._plasticity import (update_csr_on_binary_pre, update_csr_on_binary_post, update_csc_on_binary_pre,
                          update_csc_on_binary_post, update_dense_on_binary_pre, update_dense_on_binary_post,
                          update_fixed_post_conn_on_binary_pre, update_fixed_pre_conn_on_binary_post)
from ._op import OpKernel
XLACustomKernel = OpKernel      # the operator object under the reference's name (no XLA underneath)
from ._data import DataRepresentation
from ._jitc import (JITCScalarMatrix, JITCUniformMatrix, JITCNormalMatrix, JITCMatrix, JITCScalarR, JITCScalarC, JITCUniformR, JITCUniformC, JITCNormalR, JITCNormalC,
                    binary_jitsmv, binary_jitsmm, binary_jitumv, binary_jitumm, binary_jitnmv, binary_jitnmm,
                    binary_jitsmv_p, binary_jitsmm_p, binary_jitumv_p, binary_jitumm_p, binary_jitnmv_p, binary_jitnmm_p,
                    binary_jitsmv_p_call, binary_jitsmm_p_call, binary_jitumv_p_call, binary_jitumm_p_call,
                    binary_jitnmv_p_call, binary_jitnmm_p_call, JITCScatterShard, JITCGatherShard,
                    jitsmv, jitsmm, jitumv, jitumm, jitnmv, jitnmm, jitsmv_p, jitsmm_p, jitumv_p, jitumm_p, jitnmv_p, jitnmm_p,
                    jitsmv_p_call, jitsmm_p_call, jitumv_p_call, jitumm_p_call, jitnmv_p_call, jitnmm_p_call,
                    jitsmv_dt2t, jitumv_dt2t, jitnmv_dt2t, jit_param_sums)
