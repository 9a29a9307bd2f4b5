"""ctypes prototypes of the C ABI: one entry per function that ``include/brainevent_amd.h`` declares.

``PROTOTYPES[name] = (restype, (argtypes...))`` is the only place on the Python side where a C prototype is written down;
``_lib.fn`` installs it on the symbol.  An installed wheel does not carry the header, so the table is written out here and
``tests/test_abi_table_cpu.py`` compares it with the preprocessed header, name by name and argument by argument: a new entry
point needs its declaration there and one entry here (kept in the header's order, a line break at each of its sections).

A signature is ``'<return>:<arguments>'``, one letter per type.  Pointers (``be_stream_t`` included) are ``p`` unless the
callers hand in a host variable with ``byref``; those name their pointee.
"""
import ctypes as C

_TYPES = {'i': C.c_int, 'l': C.c_int64, 'u': C.c_uint32, 'd': C.c_double, 'p': C.c_void_p, 's': C.c_char_p,
          'I': C.POINTER(C.c_int), 'L': C.POINTER(C.c_int64), 'U': C.POINTER(C.c_uint32), 'Q': C.POINTER(C.c_uint64),
          'F': C.POINTER(C.c_float), 'P': C.POINTER(C.c_void_p)}

_SIGNATURES = dict(
    be_version='i:', be_last_error='s:', be_device_count='i:', be_device_max_grid_y='l:', be_build_arch='s:',
    be_profile_enable='i:i', be_profile_read='i:pi', be_diag_stream_read='i:plipFp', be_shutdown='i:',
    be_lif_coba_step='i:pppppppplddddddddddddp', be_lif_coba_step_packed='i:ppppppppplddddddddddddp',
    be_lif_cuba_step='i:pppppppplddddddddddp', be_lif_cuba_step_packed='i:ppppppppplddddddddddp',
    be_lif_step_scaled_packed='i:ippppppddppplddddddddddddp',
    be_lif_sg_forward='i:pppppplldddip', be_lif_sg_backward='i:pppppplldddiidip',
    be_lif_sg_forward_params='i:ppplplpppplldip', be_lif_sg_backward_params='i:pppppplplpppplldiidip',
    be_lif_sg_reduce_slots_workspace_bytes='l:ll', be_lif_sg_reduce_slots='i:pllpplp',
    be_lif_syn_sg_forward='i:pppppppppppllddddddiip', be_lif_syn_sg_backward='i:pppppppppppllddddddiidiip',
    be_lif_syn_sg_forward_params='i:ppppplplplplplpppppppplldiip',
    be_lif_syn_sg_backward_params='i:ppppppppppplplplplplppppppppplldiidiip',
    be_lif_rec_sg_forward='i:ppppppppppppppplllddddddiiip', be_lif_rec_sg_backward='i:ppppppppppppppplllddddddiidiip',
    be_lif_rec_sg_forward_params='i:ppppppppplplplplplppppppppllldiiip',
    be_lif_rec_sg_backward_params='i:pppppppppppppplplplplplppppppppppllldiidiip',
    be_lif_rec_delay_sg_forward='i:pppppipipppppppppplllddddddiiip',
    be_lif_rec_delay_sg_backward='i:ppppppippppppppppilllddddddiidiip',
    be_pack_spikes='i:pilpp', be_pack_spikes_batched='i:pillpp', be_unpack_spikes='i:plpp', be_compact_spikes='i:pilppp',
    be_compact_spikes_batched='i:pillplpp',
    be_exchange_unique_id_bytes='i:', be_exchange_get_unique_id='i:p', be_exchange_init='i:piilP', be_exchange_slice='i:piLL',
    be_exchange_slice_for='i:liiLLL', be_exchange_full_words='l:p', be_exchange_allgather_bits='i:ppipp',
    be_exchange_post='i:ppiip', be_exchange_wait='i:piPp', be_exchange_release='i:pip', be_exchange_post_ids='i:ppiip',
    be_exchange_wait_ids='i:pipPp', be_exchange_emulate_latency_us='i:d', be_exchange_destroy='i:p',
    be_binary_csrmv_t_workspace_bytes='l:lli', be_binary_csrmm_t_workspace_bytes='l:llli',
    be_binary_csrmv_t='i:piippilpipllplp', be_binary_csrmm_t='i:piippilpiplllplp',
    be_scatter_plan_scratch_bytes='l:llii', be_scatter_plan_count='i:ppillliiiipplLp',
    be_scatter_plan_fill='i:piippillliiipppp', be_scatter_plan_refresh_weights='i:piippillliiipppp',
    be_scatter_plan_begin='i:lliiplp', be_scatter_plan_count_rows='i:ppilllliiiipplpp', be_scatter_plan_scan='i:lliipplLp',
    be_scatter_plan_count_ordered='i:ppillliiiipplLpp', be_scatter_plan_fill_ordered='i:piippillliiippppp',
    be_scatter_plan_refresh_weights_ordered='i:piippillliiippppp', be_scatter_plan_refresh_workspace_bytes='l:l',
    be_scatter_plan_refresh_rows='i:pippillliiipppppiplp', be_scatter_plan_slots='i:pippillliiippppp',
    be_scatter_plan_patch_entries='i:pipippilplliiipppiplp', be_fixed_point_scratch_bytes='l:l', be_weight_stats='i:pilUUplp',
    be_fixed_point_exponent='i:piplliiplIp', be_scatter_plan_exponent='i:pplliiilpiiplIp',
    be_binary_csrmv_t_plan_workspace_bytes='l:lliiii', be_binary_csrmm_t_plan_workspace_bytes='l:llliiii',
    be_binary_csrmm_t_plan_workspace_bytes_for='l:llliiiii', be_binary_csrmv_t_plan='i:piipppiplliiiiiiplp',
    be_binary_csrmm_t_plan='i:piipppipllliiiiiiplp',
    be_binned_bins='i:lii', be_binned_set_tuning='i:ii', be_binned_workspace_status='i:pip', be_binned_workspace_audit='i:pQp',
    be_binary_csrmv_t_binned_workspace_bytes='l:llil', be_binary_csrmv_t_binned_workspace_init='i:plllilp',
    be_binary_csrmv_t_binned='i:piippilpiplliliplp', be_binary_csrmm_t_binned_workspace_bytes='l:lllil',
    be_binary_csrmm_t_binned_workspace_init='i:pllllilp', be_binary_csrmm_t_binned='i:piippilpipllliliplp',
    be_binary_csrmv_nt_workspace_bytes='l:ll', be_binary_csrmm_nt_workspace_bytes='l:lll',
    be_binary_csrmv_nt='i:piippilpipllplp', be_binary_csrmm_nt='i:piippilpiplllplp',
    be_csr_to_csc_scratch_bytes='l:l', be_csr_to_csc_count='i:pllpp', be_csr_to_csc_indptr='i:plpiLplp',
    be_csr_to_csc_fill_block='i:ppilllllppppipipp', be_gather_by_perm='i:pipilpp',
    be_csr_to_csc_fill_block_u8='i:ppilllllppppippp',
    be_csrmm_workspace_bytes='l:lllii', be_csrmm='i:piippilpplllliplp', be_csrmv='i:piippilppllliplp',
    be_dt2t='i:piipppilpllllip',
    be_slice_rows_tile_cols='i:i', be_slice_rows='i:piippilplplllp', be_slice_rows_grad_workspace_bytes='l:li',
    be_slice_rows_grad='i:pippilpppllpilllplp', be_slice_rows_copy='i:ppipilppllllppp',
    be_jitmm_float_workspace_bytes='l:llllii', be_jitmm_float='i:iddilupplllliiplp',
    be_jitmm_float_scatter_workspace_bytes='l:llli', be_jitmm_float_scatter='i:iddilupplllliiplp',
    be_jitmv_float='i:iddiluppllliplp',
    be_binary_csrmm_t_indexed='i:piippilpipiplllplp', be_binary_csrmm_nt_indexed='i:piippilpipiplllplp',
    be_binary_densemm_workspace_bytes='l:lllii', be_binary_densemm='i:pipipllliplp',
    be_binary_densemm_f8_workspace_bytes='l:lllii', be_binary_densemm_f8='i:pidpipllliplp',
    be_binary_csrmv_t_f8_workspace_bytes='l:ll', be_binary_csrmm_t_f8_workspace_bytes='l:lll',
    be_binary_csrmv_t_f8='i:pidppillpipllplp', be_binary_csrmm_t_f8='i:pidppillpiplllplp',
    be_binary_csrmv_nt_f8_workspace_bytes='l:ll', be_binary_csrmm_nt_f8_workspace_bytes='l:lll',
    be_binary_csrmv_nt_f8='i:pidppillpipllplp', be_binary_csrmm_nt_f8='i:pidppillpiplllplp',
    be_scatter_plan_q8_scratch_bytes='l:llii', be_scatter_plan_q8_count='i:ppillliipplLpp',
    be_scatter_plan_q8_fill='i:pppillliipppp', be_binary_csrmv_t_plan_f8_workspace_bytes='l:lliiii',
    be_binary_csrmm_t_plan_f8_workspace_bytes='l:llliiii', be_binary_csrmv_t_plan_f8='i:ppidpiplliiiiplp',
    be_binary_csrmm_t_plan_f8='i:ppidpipllliiiiplp',
    be_jit_scatter_workspace_arm='i:plp', be_jit_scatter_workspace_disarm='i:p', be_binary_jitmv_workspace_bytes='l:llli',
    be_binary_jitmv='i:iddilupipllliiplp', be_jit_scatter_classes='i:lli', be_binary_jitmv_sharded='i:iddilupipllliiiplp',
    be_binary_jitmv_rows='i:iddilupipllllplp', be_binary_jitmm_workspace_bytes='l:lllli', be_binary_jitmm='i:iddilupiplllliplp',
    be_jit_edge_weights='i:iddupplpp', be_jitc_csr_count='i:lulllipp', be_jitc_csr_fill='i:iddlulllippppp',
    be_jitc_fill_sorted='i:iddlulllippippp',
    be_plasticity_workspace_bytes='l:l', be_plasticity_rows='i:pippillpipilpididplp',
    be_plasticity_rows_aged='i:pippilpipilppliiididplp', be_plasticity_dense='i:ipillpipididplp',
    be_grad_mask_bytes='l:ll', be_grad_pack_activity='i:pillpp', be_grad_pack_activity_aged='i:ppllliipp',
    be_grad_rows_workspace_bytes='l:l',
    be_grad_rows='i:ipiippilllplpllplp', be_grad_dense_workspace_bytes='l:ll', be_grad_dense='i:ipillplpllp',
    be_sddmm_rows='i:pippilplllpplp',
    be_entries_dense_op='i:ppiippillllpillip', be_diag_scan='i:ppilllpp', be_diag_move='i:piippillpplpppip',
    be_diag_fill='i:piillpppplppp',
    be_solve_workspace_bytes='l:li', be_solve_setup='i:pippillplp', be_solve_residual='i:pippillppplp',
    be_solve_diagonal='i:ilppplp', be_solve_iterate='i:pippillpidplp',
    be_delay_split_workspace_bytes='l:li', be_delay_split_count='i:pilplipiplp', be_delay_split_fill='i:pilpplipipppp',
    be_spike_ring_push='i:pilipppp', be_spike_ring_compact='i:ppliipppp', be_value_ring_push='i:pilipippp',
    be_spike_ring_push_batch='i:pililpppp', be_spike_ring_unroll='i:pplilippp',
)

# be_binary_jit{s,u,n}{mv,mm}_{notrans,trans}_{w}: BE_FOR_JIT_VARIANTS over BE_DECL_JIT_VARIANT (BE_JIT_MV_ARGS / BE_JIT_MM_ARGS)
for _f in 'sun':
    for _w in ('f32', 'f64', 'f16', 'bf16'):
        for _t in ('notrans', 'trans'):
            _SIGNATURES[f'be_binary_jit{_f}mv_{_t}_{_w}'] = 'i:ddlupipllliplp'
            _SIGNATURES[f'be_binary_jit{_f}mm_{_t}_{_w}'] = 'i:ddlupipllllplp'

# the per-variant wrappers: BE_FOR_ALL_VARIANTS over BE_DECL_VARIANT (BE_CSR_ / BE_FCN_ / BE_DENSE_ x MV_ARGS / MM_ARGS)
for _w in ('f32', 'f64', 'f16', 'bf16'):
    for _s in ('bool', 'float'):
        for _d, _dn in (('t', 'scatter'), ('nt', 'gather')):
            for _h in ('homo', 'hetero'):
                _SIGNATURES[f'be_binary_csrmv_{_d}_{_h}_{_w}_{_s}'] = 'i:pppippllplp'
                _SIGNATURES[f'be_binary_csrmm_{_d}_{_h}_{_w}_{_s}'] = 'i:pppipplllplp'
                _SIGNATURES[f'be_binary_fcnmv_{_dn}_{_h}_{_w}_{_s}'] = 'i:pppplllplp'
                _SIGNATURES[f'be_binary_fcnmm_{_dn}_{_h}_{_w}_{_s}'] = 'i:ppppllllplp'
        for _t in ('transpose', 'no_transpose'):
            _SIGNATURES[f'be_binary_densemv_{_t}_{_w}_{_s}'] = 'i:pppllplp'
            _SIGNATURES[f'be_binary_densemm_{_t}_{_w}_{_s}'] = 'i:ppplllplp'

# declared after the variant wrappers, at the end of the header
_SIGNATURES.update(be_jit_param_grad_workspace_bytes='l:llli', be_jit_param_grad='i:iiluppllllipplp')

PROTOTYPES = {name: (_TYPES[sig[0]], tuple(_TYPES[c] for c in sig[2:])) for name, sig in _SIGNATURES.items()}
