"""The stream contract of include/zkt_plonk.h as a table: one row per entry point that takes device pointers or runs on
the context's stream.  tests/test_caller_stream_abi.py holds the table against the header (no GPU needed);
tests/test_gpu_caller_stream.py runs every row on a stream the caller keeps busy.

kind     ENQUEUE_ONLY: the call returns without waiting for the stream; SYNCHRONISES: it waits (its result goes to host
         memory, or it allocates), as the header says for that entry
words    the header's own words for that, quoted; they stand in the comment in front of the entry's declaration, or,
         with where = CONVENTIONS, in the conventions at the top of the header (the rule for every _dev entry whose own
         comment says nothing else)
reads    the caller's device buffers the call reads
writes   the caller's device buffers it writes (results in host memory are not listed)
wrapper  the zkt_plonk_amd.Context method the GPU test calls
test     the GPU test that exercises the row on a held stream
exempt   zkt_debug_* entries only: why the row has no stream test"""
from collections import namedtuple

ENQUEUE_ONLY, SYNCHRONISES = "enqueue_only", "synchronises"
OWN, CONVENTIONS = "own", "conventions"
GPU_MODULE = "test_gpu_caller_stream"

Row = namedtuple("Row", "symbol form kind words where reads writes wrapper test exempt", defaults=(None,))

_DEV_RULE = "enqueue on the context's stream without synchronising"

ROWS = [
    Row("zkt_ntt_dev", "forward, inverse with coset, in place, in_len < n", ENQUEUE_ONLY, _DEV_RULE, CONVENTIONS,
        ["d_in"], ["d_out"], "ntt_dev", "test_ntt_dev"),
    Row("zkt_debug_ntt_batch", "three transforms of one plan, one of them in place", ENQUEUE_ONLY,
        "enqueued on the context's stream", OWN, ["d_in[y]"], ["d_out[y]"], "debug_ntt_batch", "test_debug_ntt_batch"),
    Row("zkt_srs_load_dev", "a key the caller's kernel produces on the stream", SYNCHRONISES, "Synchronises the stream", OWN,
        ["d_g1_xy_mont"], [], "srs_load_dev", "test_srs_load_dev_and_msm_dev"),
    Row("zkt_msm_g1_dev", "the whole key; after four enqueued MSMs", SYNCHRONISES, "Synchronises the stream", OWN,
        ["d_scalars"], [], "msm_dev", "test_srs_load_dev_and_msm_dev"),
    Row("zkt_msm_enqueue_dev", "four back to back (a slot is reused), then zkt_msm_g1_dev", ENQUEUE_ONLY,
        "no host finish, no sync", OWN, ["d_scalars"], [], "msm_enqueue_dev", "test_msm_enqueue_dev_reuses_a_slot"),
    Row("zkt_msm_g1_bases_dev", "1000 caller bases", SYNCHRONISES, "Synchronises the stream", OWN,
        ["d_bases_xy_mont", "d_scalars"], [], "msm_bases_dev", "test_msm_bases_dev"),
    Row("zkt_kzg_commit_batch_dev", "k = 3, lengths n + 3, n / 2, 1", SYNCHRONISES, "Synchronises the stream", OWN,
        ["d_coeffs[j]"], [], "kzg_commit_batch_dev", "test_kzg_commit_batch_dev"),
    Row("zkt_kzg_open_dev", "k = 3", SYNCHRONISES, "Synchronises the stream", OWN,
        ["d_coeffs[j]"], [], "kzg_open_dev", "test_kzg_open_dev"),
    Row("zkt_commit_evals_dev", "both paths", SYNCHRONISES, "Synchronises the stream", OWN,
        ["d_evals"], [], "commit_evals_dev", "test_commit_evals_dev"),
    Row("zkt_circuit_sigma_dev", "n = 128", SYNCHRONISES, "synchronises once, at the end", OWN,
        ["d_w_l", "d_w_r", "d_w_o"], ["d_sigma[3]"], "circuit_sigma", "test_circuit_sigma_dev"),
    Row("zkt_circuit_check_witness", "device wires and device variables plus wiring, satisfied and broken", SYNCHRONISES,
        "synchronises once, at the end", OWN,
        ["a_evals", "b_evals", "c_evals", "variables", "w_l", "w_r", "w_o"], [], "check_witness", "test_check_witness_on_device_inputs"),
    Row("zkt_prove", "device wires, successors announced, both quotient routes", SYNCHRONISES, "Synchronises the stream", OWN,
        ["a_evals", "b_evals", "c_evals"], [], "prove_prepared", "test_proof_chain_device_wires"),
    Row("zkt_prove", "device variables plus wiring, successors announced, both quotient routes", SYNCHRONISES,
        "Synchronises the stream", OWN, ["variables", "w_l", "w_r", "w_o"], [], "prove_prepared", "test_proof_chain_device_variables"),
    Row("zkt_prove_set_next", "the successor's device witness is written behind the hold of the proof that reads it early",
        ENQUEUE_ONLY, "nothing is enqueued, no synchronisation", OWN,
        ["a_evals", "b_evals", "c_evals", "variables", "w_l", "w_r", "w_o"], [], "prove_prepared", "test_proof_chain_device_wires"),
    Row("zkt_poseidon_hash_batch_dev", "batch 300, arity 2, BN254 x3 tables, with the round states", ENQUEUE_ONLY,
        "enqueues on the context's stream without synchronising", OWN, ["d_inputs"], ["d_out_hashes", "d_out_states"],
        "poseidon_hash_batch_dev", "test_poseidon_hash_batch_dev"),
    Row("zkt_poseidon_gadget_witness_dev", "input values and input variables", ENQUEUE_ONLY, "no allocation, no synchronisation", OWN,
        ["d_inputs", "d_input_vars", "d_variables", "d_trace_base"], ["d_variables", "d_out_hashes"],
        "poseidon_gadget_witness_dev", "test_poseidon_gadget_witness_dev"),
    Row("zkt_poseidon_merkle_path_witness_dev", "height 8", ENQUEUE_ONLY, "no allocation, no synchronisation", OWN,
        ["d_variables", "d_leaf_var", "d_bit_vars", "d_sibling_vars", "d_path_base"], ["d_variables", "d_out_roots"],
        "poseidon_merkle_path_witness_dev", "test_poseidon_merkle_path_witness_dev"),
    Row("zkt_merkle_tree_append_dev", "height 8, 37 leaves then 64 more", ENQUEUE_ONLY, "Enqueue only: no allocation, no synchronisation", OWN,
        ["d_leaves"], [], "merkle_tree_append_dev", "test_merkle_tree_append_and_paths"),
    Row("zkt_merkle_tree_paths_to_variables_dev", "5 then 7 indices back to back (the pinned table changes hands)", ENQUEUE_ONLY,
        "Enqueue only: no allocation, no synchronisation of the stream", OWN, [], ["d_variables"],
        "merkle_tree_paths_to_variables_dev", "test_merkle_tree_append_and_paths"),
    Row("zkt_g1_decompress_dev", "n = 65, every status", ENQUEUE_ONLY, "only enqueues", OWN,
        ["d_compressed"], ["d_out_xy_mont", "d_out_status"], "g1_decompress_dev", "test_g1_decompress_dev"),
    Row("zkt_verify_batch_dev", "three proofs, accepted and rejected", SYNCHRONISES, "Synchronises the stream", OWN,
        [], [], "verify_batch_dev", "test_verify_batch_dev"),
    Row("zkt_verify_batch_prepare_dev", "three proofs", SYNCHRONISES, "Synchronises the stream", OWN,
        [], [], "verify_batch_prepare_dev", "test_verify_batch_dev"),
    Row("zkt_debug_commit_wires_dev", "", SYNCHRONISES, "Synchronises the stream", OWN, ["d_variables", "d_w_l", "d_w_r", "d_w_o"], [],
        None, None, "a test hook around the prover's round 1: the same launches run, on a held stream, in every proof of the "
                    "device-variables chain (test_proof_chain_device_variables)"),
    Row("zkt_debug_commit_wires_pi_dev", "", SYNCHRONISES, "Synchronises the stream", OWN, ["d_variables", "d_w_l", "d_w_r", "d_w_o"], [],
        None, None, "the same hook with public-input positions; see zkt_debug_commit_wires_dev"),
]

# the entries the table must hold besides every zkt_*_dev symbol of the header
REQUIRED = ("zkt_debug_ntt_batch", "zkt_prove", "zkt_prove_set_next", "zkt_circuit_check_witness")

# how the header says it (matched against a row's words)
WORDS_OF = {
    ENQUEUE_ONLY: (r"without synchronising", r"no synchronisation", r"only enqueues", r"Enqueue only", r"no sync\b",
                   r"enqueued on the context's stream"),
    SYNCHRONISES: (r"Synchronises the stream", r"synchronises once, at the end", r"Synchronises\."),
}
