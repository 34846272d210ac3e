//! Raw declarations of include/zkt_plonk.h (the subset the shim uses).  Field elements cross as arkworks'
//! in-memory Montgomery limbs (`Fp256` = `BigInteger256([u64; 4])`), points as x limbs || y limbs, (0, 0) = infinity.
use std::os::raw::{c_char, c_int, c_void};

#[repr(C)]
pub struct ZktCtx {
    _private: [u8; 0],
}

#[repr(C)]
pub struct ZktTranscriptVtable {
    pub user: *mut c_void,
    pub append_u64: extern "C" fn(*mut c_void, *const c_char, u64),
    pub append_scalars: extern "C" fn(*mut c_void, *const c_char, *const u64, usize, c_int),
    pub append_commitment: extern "C" fn(*mut c_void, *const c_char, *const u64, c_int),
    pub challenge_scalar: extern "C" fn(*mut c_void, *const c_char, *mut u64),
}

#[repr(C)]
pub struct ZktCommVtable {
    pub user: *mut c_void,
    pub rank: c_int,
    pub world: c_int,
    pub device_buffers: c_int,
    pub all_gather: extern "C" fn(*mut c_void, *const c_void, *mut c_void, usize, c_int, *mut c_void) -> c_int,
    /// optional stream-ordered form for device buffers (None: the library uses the blocking callback)
    pub all_gather_async: Option<extern "C" fn(*mut c_void, *const c_void, *mut c_void, usize, *mut c_void) -> c_int>,
}

#[repr(C)]
pub struct ZktProveInputs {
    pub a_evals: *const u64,
    pub b_evals: *const u64,
    pub c_evals: *const u64,
    pub n_rows: usize,
    pub table: *const u64,
    pub table_len: usize,
    pub pi_pos: *const usize,
    pub pi_vals: *const u64,
    pub n_pi: usize,
    pub blinders: *const u64,
    pub wires_on_device: c_int,
    pub variables: *const u64,
    pub n_vars: usize,
    pub w_l: *const u32,
    pub w_r: *const u32,
    pub w_o: *const u32,
}

/// zkt_witness_report: what zkt_circuit_check_witness found (check_gate, constraint_system/helper.rs:13-75, every row)
#[repr(C)]
pub struct ZktWitnessReport {
    pub satisfied: c_int,
    pub checked: c_int,
    pub n_arithmetic: u64,
    pub first_arithmetic: u64,
    pub residual: [u64; 4],
    pub n_lookup: u64,
    pub first_lookup: u64,
    pub n_wiring: u64,
    pub first_wiring_row: u64,
    pub first_wiring_column: c_int,
}

/// zkt_srs_report: what zkt_srs_check found in a committer key (per-point statuses, then the structure test)
#[repr(C)]
pub struct ZktSrsReport {
    pub count: u64,
    pub n_bad: u64,
    pub first_bad: u64,
    pub by_status: [u64; 6],
    pub first_bad_status: c_int,
    pub points_ok: c_int,
    pub structure_checked: c_int,
    pub structure_ok: c_int,
    pub ok: c_int,
    pub sum_xy_mont: [u64; 12],
    pub sum_is_infinity: c_int,
}

pub const ZKT_CHECK_WIRING: c_int = 1;
pub const ZKT_CHECK_NONE: u64 = u64::MAX;
pub const ZKT_VARIABLE_ZERO: u32 = 0xFFFF_FFFF;
pub const ZKT_CURVE_BN254: c_int = 0;
pub const ZKT_CURVE_BLS12_381: c_int = 1;
pub const ZKT_KZG_BATCH_MAX: usize = 32;   // include/zkt_plonk.h: most polynomials per zkt_kzg_commit_batch / zkt_kzg_open

extern "C" {
    pub fn zkt_ctx_create(curve_id: c_int, device_id: c_int, out: *mut *mut ZktCtx) -> c_int;
    pub fn zkt_ctx_destroy(ctx: *mut ZktCtx);
    pub fn zkt_last_error(ctx: *const ZktCtx) -> *const c_char;
    pub fn zkt_ctx_set_comm(ctx: *mut ZktCtx, comm: *const ZktCommVtable) -> c_int;
    pub fn zkt_shard_range(total: usize, rank: c_int, world: c_int, lo: *mut usize, hi: *mut usize) -> c_int;
    pub fn zkt_ntt(ctx: *mut ZktCtx, log_n: c_int, inverse: c_int, coset: c_int, input: *const u64, in_len: usize,
                   out: *mut u64) -> c_int;
    pub fn zkt_srs_load(ctx: *mut ZktCtx, g1_xy_mont: *const u64, count: usize) -> c_int;
    pub fn zkt_srs_load_slice(ctx: *mut ZktCtx, g1_xy_mont: *const u64, offset: usize, count: usize, total: usize) -> c_int;
    pub fn zkt_srs_load_file(ctx: *mut ZktCtx, ck_path: *const c_char, max_powers: usize) -> c_int;
    pub fn zkt_msm_g1(ctx: *mut ZktCtx, scalars: *const u64, len: usize, base_offset: usize, scalars_montgomery: c_int,
                      out_xy_mont: *mut u64, out_is_infinity: *mut c_int) -> c_int;
    pub fn zkt_ctx_fork(ctx: *mut ZktCtx, out: *mut *mut ZktCtx) -> c_int;
    pub fn zkt_kzg_commit_batch(ctx: *mut ZktCtx, coeffs: *const *const u64, lens: *const usize, k: c_int,
                                scalars_montgomery: c_int, out_xy_mont: *mut u64, out_is_infinity: *mut c_int) -> c_int;
    pub fn zkt_kzg_commit_batch_dev(ctx: *mut ZktCtx, d_coeffs: *const *const c_void, lens: *const usize, k: c_int,
                                    scalars_montgomery: c_int, out_xy_mont: *mut u64, out_is_infinity: *mut c_int) -> c_int;
    pub fn zkt_kzg_open(ctx: *mut ZktCtx, coeffs: *const *const u64, lens: *const usize, k: c_int, challenges_mont: *const u64,
                        point_mont: *const u64, out_w_xy_mont: *mut u64, out_w_is_infinity: *mut c_int,
                        out_evals_mont: *mut u64) -> c_int;
    pub fn zkt_kzg_open_dev(ctx: *mut ZktCtx, d_coeffs: *const *const c_void, lens: *const usize, k: c_int,
                            challenges_mont: *const u64, point_mont: *const u64, out_w_xy_mont: *mut u64,
                            out_w_is_infinity: *mut c_int, out_evals_mont: *mut u64) -> c_int;
    pub fn zkt_commit_evals_dev(ctx: *mut ZktCtx, d_evals: *const c_void, blinders: *const u64, k: c_int, path: c_int,
                                out_xy_mont: *mut u64, out_is_infinity: *mut c_int) -> c_int;
    pub fn zkt_ctx_set_lagrange(ctx: *mut ZktCtx, on: c_int) -> c_int;
    pub fn zkt_ctx_set_wire_elimination(ctx: *mut ZktCtx, mode: c_int) -> c_int;
    pub fn zkt_ctx_set_quotient_route(ctx: *mut ZktCtx, mode: c_int) -> c_int;
    pub fn zkt_ctx_set_fused_passes(ctx: *mut ZktCtx, mode: c_int) -> c_int;
    pub fn zkt_ctx_set_verify_terms(ctx: *mut ZktCtx, mode: c_int) -> c_int;
    pub fn zkt_lagrange_info(ctx: *mut ZktCtx, log_n: *mut c_int, bases: *mut usize) -> c_int;
    pub fn zkt_circuit_load(ctx: *mut ZktCtx, log_n: c_int, pk_polys: *const *const u64, pk_lens: *const usize) -> c_int;
    pub fn zkt_circuit_load_file(ctx: *mut ZktCtx, pk_path: *const c_char, log_n: c_int) -> c_int;
    pub fn zkt_keyfile_extended_prover_key(path: *const c_char, curve_id: c_int, which: c_int, out_mont: *mut u64, cap: usize,
                                           lens17: *mut usize) -> c_int;
    pub fn zkt_circuit_check_epk_file(ctx: *mut ZktCtx, epk_path: *const c_char, first_mismatch_vector: *mut c_int,
                                      mismatch_at: *mut usize) -> c_int;
    pub fn zkt_circuit_setup(ctx: *mut ZktCtx, log_n: c_int, evals: *const *const u64, eval_lens: *const usize,
                             evals_on_device: c_int, out_commitments: *mut u64, out_is_infinity: *mut c_int) -> c_int;
    pub fn zkt_circuit_sigma_dev(ctx: *mut ZktCtx, log_n: c_int, d_w_l: *const u32, d_w_r: *const u32, d_w_o: *const u32,
                                 n_rows: usize, n_vars: usize, d_sigma: *const *mut c_void) -> c_int;
    pub fn zkt_circuit_setup_wiring(ctx: *mut ZktCtx, log_n: c_int, evals: *const *const u64, eval_lens: *const usize,
                                    evals_on_device: c_int, w_l: *const u32, w_r: *const u32, w_o: *const u32, n_rows: usize,
                                    n_vars: usize, wiring_on_device: c_int, out_commitments: *mut u64,
                                    out_is_infinity: *mut c_int) -> c_int;
    pub fn zkt_prove_with(ctx: *mut ZktCtx, inputs: *const ZktProveInputs, transcript: *const ZktTranscriptVtable,
                          proof_out: *mut u8, proof_cap: usize, proof_len: *mut usize) -> c_int;
    pub fn zkt_prove_set_next(ctx: *mut ZktCtx, next: *const ZktProveInputs) -> c_int;
    pub fn zkt_circuit_check_witness(ctx: *mut ZktCtx, inputs: *const ZktProveInputs, flags: c_int,
                                     out: *mut ZktWitnessReport) -> c_int;
    pub fn zkt_g1_msm_host(curve_id: c_int, points_xy_mont: *const u64, scalars: *const u64, n: usize, scalars_montgomery: c_int,
                           out_xy_mont: *mut u64, out_is_infinity: *mut c_int) -> c_int;
    pub fn zkt_msm_g1_bases(ctx: *mut ZktCtx, bases_xy_mont: *const u64, scalars: *const u64, n: usize,
                            scalars_montgomery: c_int, out_xy_mont: *mut u64, out_is_infinity: *mut c_int) -> c_int;
    pub fn zkt_msm_g1_bases_dev(ctx: *mut ZktCtx, d_bases_xy_mont: *const c_void, d_scalars: *const c_void, n: usize,
                                scalars_montgomery: c_int, out_xy_mont_host: *mut u64, out_is_infinity: *mut c_int) -> c_int;
    pub fn zkt_verify(curve_id: c_int, inputs: *const ZktVerifyInputs, transcript: *mut c_void, h_g2_mont: *const u64,
                      beta_h_g2_mont: *const u64, accepted: *mut c_int) -> c_int;
    pub fn zkt_verify_batch(curve_id: c_int, inputs: *const ZktVerifyInputs, transcripts: *const *mut c_void, count: usize,
                            h_g2_mont: *const u64, beta_h_g2_mont: *const u64, accepted: *mut c_int) -> c_int;
    pub fn zkt_verify_batch_prepare_dev(ctx: *mut ZktCtx, inputs: *const ZktVerifyInputs, transcripts: *const *mut c_void, count: usize,
                                        h_g2_mont: *const u64, beta_h_g2_mont: *const u64, out_ab: *mut u64,
                                        out_ab_is_infinity: *mut c_int, out_rho: *mut u64) -> c_int;
    pub fn zkt_verify_batch_dev(ctx: *mut ZktCtx, inputs: *const ZktVerifyInputs, transcripts: *const *mut c_void, count: usize,
                                h_g2_mont: *const u64, beta_h_g2_mont: *const u64, accepted: *mut c_int) -> c_int;
    pub fn zkt_verify_batch_locate(ctx: *mut ZktCtx, inputs: *const ZktVerifyInputs, transcripts: *const *mut c_void, count: usize,
                                   h_g2_mont: *const u64, beta_h_g2_mont: *const u64, accepted: *mut c_int, out_bad: *mut u8,
                                   n_bad: *mut usize, n_checks: *mut usize) -> c_int;
    pub fn zkt_g1_decompress(ctx: *mut ZktCtx, compressed: *const u8, n: usize, out_xy_mont: *mut u64, out_status: *mut u8) -> c_int;
    pub fn zkt_g1_decompress_dev(ctx: *mut ZktCtx, d_compressed: *const c_void, n: usize, d_out_xy_mont: *mut c_void,
                                 d_out_status: *mut c_void) -> c_int;
    pub fn zkt_g1_check(ctx: *mut ZktCtx, points_xy_mont: *const c_void, n: usize, points_on_device: c_int, out_status: *mut u8) -> c_int;
    pub fn zkt_srs_check(ctx: *mut ZktCtx, g1_xy_mont: *const c_void, count: usize, points_on_device: c_int, h_g2_mont: *const u64,
                         beta_h_g2_mont: *const u64, seed32: *const u8, out_status: *mut u8, report: *mut ZktSrsReport) -> c_int;
    pub fn zkt_poseidon_load(ctx: *mut ZktCtx, params: *const ZktPoseidonParams, out: *mut *mut c_void) -> c_int;
    pub fn zkt_poseidon_free(ctx: *mut ZktCtx, params: *mut c_void);
    pub fn zkt_poseidon_hash_batch_dev(ctx: *mut ZktCtx, params: *const c_void, d_inputs: *const c_void, batch: usize,
                                       arity: c_int, d_out_hashes: *mut c_void, d_out_states: *mut c_void) -> c_int;
    pub fn zkt_poseidon_gadget_vars_per_hash(params: *const c_void) -> usize;
    pub fn zkt_poseidon_gadget_witness_dev(ctx: *mut ZktCtx, params: *const c_void, args: *const ZktPoseidonGadgetArgs) -> c_int;
    pub fn zkt_poseidon_gadget_check(ctx: *mut ZktCtx, params: *const c_void) -> c_int;
    pub fn zkt_merkle_path_vars_per_level(params: *const c_void) -> usize;
    pub fn zkt_poseidon_merkle_path_witness_dev(ctx: *mut ZktCtx, params: *const c_void, args: *const ZktMerklePathArgs) -> c_int;
    pub fn zkt_poseidon_merkle_path_validate(ctx: *mut ZktCtx, params: *const c_void, args: *const ZktMerklePathArgs) -> c_int;
    // the note tree (gadgets/src/merkle_tree.rs) kept on the device; `tree` is the opaque zkt_merkle_tree
    pub fn zkt_merkle_tree_create(ctx: *mut ZktCtx, params: *const c_void, height: c_int, capacity: usize, out: *mut *mut c_void) -> c_int;
    pub fn zkt_merkle_tree_free(ctx: *mut ZktCtx, tree: *mut c_void);
    pub fn zkt_merkle_tree_append_dev(ctx: *mut ZktCtx, tree: *mut c_void, d_leaves: *const c_void, m: usize, first_index: *mut u64) -> c_int;
    pub fn zkt_merkle_tree_append(ctx: *mut ZktCtx, tree: *mut c_void, leaves: *const u64, m: usize, first_index: *mut u64) -> c_int;
    pub fn zkt_merkle_tree_root(ctx: *mut ZktCtx, tree: *mut c_void, out4: *mut u64) -> c_int;
    pub fn zkt_merkle_tree_info(tree: *const c_void, height: *mut c_int, count: *mut u64, capacity: *mut u64) -> c_int;
    pub fn zkt_merkle_tree_layer(ctx: *mut ZktCtx, tree: *mut c_void, layer: c_int, first: u64, n: usize, out: *mut u64) -> c_int;
    pub fn zkt_merkle_tree_paths(ctx: *mut ZktCtx, tree: *mut c_void, indices: *const u64, k: usize, out_siblings: *mut u64) -> c_int;
    pub fn zkt_merkle_tree_paths_to_variables_dev(ctx: *mut ZktCtx, tree: *mut c_void, indices: *const u64, k: usize,
                                                  d_variables: *mut c_void, n_vars: usize, bit_var0: *const u32,
                                                  sibling_var0: *const u32) -> c_int;
    pub fn zkt_debug_merkle_tree_split(tree: *mut c_void, wide_min_parents: c_int) -> c_int;
    // the reference CLI's store files (--merkle-tree, --notes): include/zkt_plonk.h "(4b) The store files"
    pub fn zkt_merkle_tree_save_file(ctx: *mut ZktCtx, tree: *mut c_void, path: *const c_char) -> c_int;
    pub fn zkt_merkle_tree_load_file(ctx: *mut ZktCtx, poseidon: *const c_void, height: c_int, capacity: usize, path: *const c_char,
                                     out: *mut *mut c_void, report: *mut ZktTreeFileReport) -> c_int;
    pub fn zkt_notes_read_file(path: *const c_char, curve_id: c_int, cap: usize, out_leaf_indices: *mut u64,
                               out_identifiers_mont: *mut u64, out_amounts: *mut u64, out_secrets_mont: *mut u64,
                               count: *mut usize) -> c_int;
    pub fn zkt_notes_write_file(path: *const c_char, curve_id: c_int, leaf_indices: *const u64, identifiers_mont: *const u64,
                                amounts: *const u64, secrets_mont: *const u64, count: usize) -> c_int;
    pub fn zkt_debug_store_chunk(ctx: *mut ZktCtx, nodes: usize) -> c_int;
    pub fn zkt_debug_live_allocations(count: *mut u64, bytes: *mut u64) -> c_int;
    pub fn zkt_dev_alloc(ctx: *mut ZktCtx, bytes: usize, dptr: *mut *mut c_void) -> c_int;
    pub fn zkt_dev_free(ctx: *mut ZktCtx, dptr: *mut c_void) -> c_int;
    pub fn zkt_dev_upload(ctx: *mut ZktCtx, dptr: *mut c_void, host: *const c_void, bytes: usize) -> c_int;
    // the withdraw circuit as a component (include/zkt_plonk.h "(5) The withdraw circuit")
    pub fn zkt_withdraw_create(ctx: *mut ZktCtx, params: *const ZktPoseidonParams, inputs: c_int, height: c_int, out: *mut *mut c_void) -> c_int;
    pub fn zkt_withdraw_free(ctx: *mut ZktCtx, w: *mut c_void);
    pub fn zkt_withdraw_poseidon(w: *const c_void) -> *const c_void;
    pub fn zkt_withdraw_get_info(w: *const c_void, out: *mut ZktWithdrawInfo) -> c_int;
    pub fn zkt_withdraw_pi_pos(w: *const c_void, out: *mut usize) -> c_int;
    pub fn zkt_withdraw_rows(ctx: *mut ZktCtx, w: *const c_void, out_selectors6: *const *mut u64, out_wires3: *const *mut u32) -> c_int;
    pub fn zkt_debug_withdraw_layout_host(curve_id: c_int, params: *const ZktPoseidonParams, inputs: c_int, height: c_int,
                                          info: *mut ZktWithdrawInfo, out_selectors6: *const *mut u64, out_wires3: *const *mut u32,
                                          out_pi_pos: *mut usize, out_hash_calls: *mut u32) -> c_int;
    pub fn zkt_withdraw_setup(ctx: *mut ZktCtx, w: *const c_void, log_n: c_int, table_size: usize, out_commitments: *mut u64,
                              out_is_infinity: *mut c_int) -> c_int;
    pub fn zkt_withdraw_witness(ctx: *mut ZktCtx, w: *mut c_void, reqs: *const ZktWithdrawRequest, batch: usize, tree: *mut c_void,
                                d_variables: *mut c_void, stride: usize, out_pi: *mut u64, out_status: *mut ZktWithdrawStatus) -> c_int;
    pub fn zkt_withdraw_prove_inputs(w: *const c_void, d_variables: *const c_void, stride: usize, b: usize, pi_pos: *const usize,
                                     pi_vals: *const u64, out: *mut ZktProveInputs) -> c_int;
    pub fn zkt_note_leaves(ctx: *mut ZktCtx, poseidon: *const c_void, d_secrets: *const c_void, d_identifiers: *const c_void,
                           d_amounts_u64: *const c_void, m: usize, d_out_leaves: *mut c_void) -> c_int;
    // ProveWithdraw in one call: witness, proofs, their check and the append of the new leaves
    pub fn zkt_withdraw_prove(ctx: *mut ZktCtx, w: *mut c_void, reqs: *const ZktWithdrawRequest, batch: usize, tree: *mut c_void,
                              args: *const ZktWithdrawProveArgs, proofs: *mut u8, proof_stride: usize, out_pi: *mut u64,
                              results: *mut ZktWithdrawResult) -> c_int;
}

/// include/zkt_comm_rccl.h: the optional RCCL transport (libzkt_comm_rccl.so), INTEGRATION.md section 3c
/// Behind the `rccl` cargo feature: a host without librccl builds and links the shim without it.
#[cfg(feature = "rccl")]
#[link(name = "zkt_comm_rccl")]
extern "C" {
    pub fn zkt_comm_rccl_unique_id(out: *mut u8) -> c_int;
    pub fn zkt_comm_rccl_create(id: *const u8, rank: c_int, world: c_int, device: c_int, out: *mut *mut c_void) -> c_int;
    pub fn zkt_comm_rccl_vtable(comm: *mut c_void, out: *mut ZktCommVtable) -> c_int;
    pub fn zkt_comm_rccl_destroy(comm: *mut c_void);
    pub fn zkt_comm_rccl_last_error(comm: *const c_void) -> *const c_char;
}

#[repr(C)]
pub struct ZktPoseidonGadgetArgs {
    pub batch: usize,
    pub arity: c_int,
    pub d_inputs: *const c_void,
    pub d_input_vars: *const u32,
    pub d_variables: *mut c_void,
    pub n_vars: usize,
    pub d_trace_base: *const u32,
    pub trace_base0: usize,
    pub d_out_hashes: *mut c_void,
    pub kernel: c_int,
}

#[repr(C)]
pub struct ZktMerklePathArgs {
    pub batch: usize,
    pub height: c_int,
    pub d_variables: *mut c_void,
    pub n_vars: usize,
    pub d_leaf_var: *const u32,
    pub d_bit_vars: *const u32,
    pub d_sibling_vars: *const u32,
    pub d_path_base: *const u32,
    pub path_base0: usize,
    pub d_out_roots: *mut c_void,
}

#[repr(C)]
pub struct ZktVerifyInputs {
    pub n: u64,
    pub vk_commitments: *const u64,
    pub vk_is_infinity: *const c_int,
    pub pi_roots: *const u64,
    pub pub_inputs: *const u64,
    pub n_pi: usize,
    pub proof: *const u8,
    pub proof_len: usize,
    pub g: *const u64,
}

#[repr(C)]
pub struct ZktPoseidonParams {
    pub width: c_int,
    pub half_full_rounds: c_int,
    pub partial_rounds: c_int,
    pub round_constants: *const u64,
    pub mds: *const u64,
    pub domain_tag: *const u64,
}

#[repr(C)]
pub struct ZktWithdrawInfo {
    pub inputs: c_int,
    pub height: c_int,
    pub width: c_int,
    pub log_n_min: c_int,
    pub n_gates: usize,
    pub n_vars: usize,
    pub n_hashes: usize,
    pub vars_per_hash: usize,
    pub n_pi: usize,
    pub device_bytes: usize,
}

#[repr(C)]
pub struct ZktWithdrawRequest {
    pub secrets: *const u64,
    pub identifiers: *const u64,
    pub amounts: *const u64,
    pub leaf_indices: *const u64,
    pub siblings: *const u64,
    pub root: *const u64,
    pub new_secret: *const u64,
    pub new_identifier: *const u64,
    pub withdraw_amount: u64,
}

#[repr(C)]
pub struct ZktWithdrawStatus {
    pub bad_paths: u32,
}

/// zkt_withdraw_prove_args
#[repr(C)]
pub struct ZktWithdrawProveArgs {
    pub transcript_kind: c_int,
    pub label: *const c_char,
    pub identifiers_set: *const u64,
    pub set_len: usize,
    pub blinders: *const u64,
    pub verify: c_int,
    pub g_xy_mont: *const u64,
    pub h_g2_mont: *const u64,
    pub beta_h_g2_mont: *const u64,
    pub append: c_int,
    pub d_variables: *mut c_void,
    pub stride: usize,
    pub slots: usize,
}

/// zkt_withdraw_result
#[repr(C)]
pub struct ZktWithdrawResult {
    pub code: c_int,
    pub bad_paths: u32,
    pub verified: c_int,
    pub new_leaf_index: u64,
}

/// zkt_tree_file_report: how a MerkleTreeStore file compares with the tree rebuilt from its leaves
#[repr(C)]
pub struct ZktTreeFileReport {
    pub entries: u64,
    pub mismatches: u64,
    pub first_layer: c_int,
    pub first_idx: u64,
    pub root_matches: c_int,
}
