// The entries that read the loaded circuit's keys for a witness: zkt_circuit_check_witness[_batch] (check.hip) and
// zkt_witness_plan_create[_ex] (witness_plan.hip).  They validate the caller's arguments against the circuit and hand the
// keys on; they write nothing of the circuit state: the work buffers, the resident lookup keys and an announced proof's
// early rounds stay as they are.  Host only.
#include "circuit.hpp"

namespace zkt {

// the keys a check reads; a plan reads the first of them (the selectors' coefficients)
static WitnessCheckKeys witness_check_keys(const CircuitState& S) {
    WitnessCheckKeys keys{};
    keys.log_n = S.log_n;
    for (int k = 0; k < 5; ++k) keys.pk[k] = S.pk[PK_QM + k];   // PK_QM .. PK_QC
    keys.q_lookup_ev = S.q_lookup_ev;
    for (int k = 0; k < 3; ++k) keys.sigma_ev[k] = S.sigma_ev[k];
    return keys;
}
static WitnessPlanKeys witness_plan_keys(const CircuitState& S) {
    const WitnessCheckKeys k = witness_check_keys(S);
    return WitnessPlanKeys{k.log_n, {k.pk[0], k.pk[1], k.pk[2], k.pk[3], k.pk[4]}};
}

// What the single check and the batch refuse alike, in the order both report it: first the call itself ...
static int refuse_check_call(zkt_ctx* c, const void* in, const void* out, int flags) {
    if (!c) return ZKT_ERR_INVALID_ARGUMENT;
    if (!in || !out) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "null pointer");
    if (int rc = circuit_entry(c, 0)) return rc;
    if (flags & ~ZKT_CHECK_WIRING) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "unknown flag bits");
    return ZKT_OK;
}
// ... then the rows, the lookup tables (host) and the public inputs against the circuit bound n ...
static int refuse_check_shape(zkt_ctx* c, size_t n, size_t n_rows, const uint64_t* const* tables, const size_t* table_lens,
                              size_t n_tables, const size_t* pi_pos, const void* pi_vals, size_t n_pi) {
    if (n_rows > n) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "more rows than the circuit bound");
    for (size_t t = 0; t < n_tables; ++t) {
        if (table_lens[t] >= n) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "max table size is equal or larger than n");
        if (table_lens[t] && !tables[t]) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "null lookup table");
    }
    if (n_pi && (!pi_pos || !pi_vals)) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "null public inputs");
    for (size_t i = 0; i < n_pi; ++i)
        if (pi_pos[i] >= n) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "public input position out of range");
    return ZKT_OK;
}
// ... and last the witness in its index form: a variable map and the wiring
static int refuse_index_form(zkt_ctx* c, const CircuitState& S, int flags, size_t n_rows, const uint32_t* w_l, const uint32_t* w_r,
                             const uint32_t* w_o, const void* variables, size_t n_vars) {
    if (n_rows && (!w_l || !w_r || !w_o)) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "null wire index vector");
    if (n_vars && !variables) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "null variable map");
    if (n_vars > 0xFFFFFFFEull) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "too many variables");
    if ((flags & ZKT_CHECK_WIRING) && S.log_n > 25)
        return set_err(c, ZKT_ERR_INVALID_DOMAIN_SIZE, "InvalidEvalDomainSize: the wiring's positions are 32-bit (log_n <= 25)");
    return ZKT_OK;
}

}  // namespace zkt

using namespace zkt;

extern "C" {

// helper.rs:13-75 check_gate over every row (check.hip)
int zkt_circuit_check_witness(zkt_ctx* c, const zkt_prove_inputs* in, int flags, zkt_witness_report* out) {
    if (int rc = refuse_check_call(c, in, out, flags)) return rc;
    const CircuitState& S = *c->circuit;
    if (int rc = refuse_check_shape(c, S.n, in->n_rows, &in->table, &in->table_len, 1, in->pi_pos, in->pi_vals, in->n_pi)) return rc;
    if (in->a_evals) {
        if (flags & ZKT_CHECK_WIRING)
            return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "ZKT_CHECK_WIRING needs the witness as variables + w_l / w_r / w_o: evaluation vectors carry no wiring");
        if (in->n_rows && (!in->b_evals || !in->c_evals)) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "null wire vector");
    } else if (int rc = refuse_index_form(c, S, flags, in->n_rows, in->w_l, in->w_r, in->w_o, in->variables, in->n_vars)) {
        return rc;
    }
    (void)hipSetDevice(c->device);
    return witness_check(c, witness_check_keys(S), *in, flags, out);
}

// The single check's rules over a batch of completed maps under one wiring (check.hip)
int zkt_circuit_check_witness_batch(zkt_ctx* c, const zkt_witness_batch* in, int flags, zkt_witness_report* out) {
    if (int rc = refuse_check_call(c, in, out, flags)) return rc;
    const CircuitState& S = *c->circuit;
    if (in->batch < 1 || in->batch > ZKT_WITNESS_BATCH_MAX) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "1 <= batch <= ZKT_WITNESS_BATCH_MAX");
    if (in->stride < in->n_vars) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "stride below n_vars");
    if (in->n_tables != 0 && in->n_tables != 1 && in->n_tables != in->batch)
        return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "n_tables must be 0, 1 or batch");
    if (in->n_tables && (!in->tables || !in->table_lens)) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "null lookup tables");
    if (int rc = refuse_check_shape(c, S.n, in->n_rows, in->tables, in->table_lens, in->n_tables, in->pi_pos, in->d_pi_vals, in->n_pi))
        return rc;
    if (int rc = refuse_index_form(c, S, flags, in->n_rows, in->w_l, in->w_r, in->w_o, in->d_variables, in->n_vars)) return rc;
    (void)hipSetDevice(c->device);
    return witness_check_batch(c, witness_check_keys(S), *in, flags, out);
}

// The plan of a witness completion over the loaded circuit's selectors (witness_plan.hip); the plan keeps no pointer into
// the circuit state.
int zkt_witness_plan_create_ex(zkt_ctx* c, const uint32_t* w_l, const uint32_t* w_r, const uint32_t* w_o, size_t n_rows, size_t n_vars,
                               int wiring_on_device, const size_t* pi_pos, size_t n_pi, uint32_t rules, zkt_witness_plan** out) {
    if (!c) return ZKT_ERR_INVALID_ARGUMENT;
    if (!out) return set_err(c, ZKT_ERR_INVALID_ARGUMENT, "null pointer");
    if (int rc = circuit_entry(c, 0)) return rc;
    return witness_plan_create(c, witness_plan_keys(*c->circuit), w_l, w_r, w_o, n_rows, n_vars, wiring_on_device, pi_pos, n_pi, rules, out);
}

int zkt_witness_plan_create(zkt_ctx* c, const uint32_t* w_l, const uint32_t* w_r, const uint32_t* w_o, size_t n_rows, size_t n_vars,
                            int wiring_on_device, const size_t* pi_pos, size_t n_pi, zkt_witness_plan** out) {
    return zkt_witness_plan_create_ex(c, w_l, w_r, w_o, n_rows, n_vars, wiring_on_device, pi_pos, n_pi, 0, out);
}

}  // extern "C"
