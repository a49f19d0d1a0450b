// chain.hpp -- the layered GKR chain that grandproduct/ and fracsum/ run, both sides of its transcript stated once: n - 1 product
// sumchecks (pks proofs), layer d's over d variables, tied by an outer transcript
//     bind | top | rho | per layer d = 1 .. n - 1: the layer's challenges | [its pks proof] | its finals | rho
// in a proof  top | layer 1's pks proof | .. | layer n - 1's, whose last elements are the layer's finals.  The point z_d of layer d's eq
// factor is (rho, r_{d-1}): the challenge after layer d - 1's finals in front of that layer's sumcheck point.
//
// What differs between a tree of products and a tree of fractions is a *rule*, which the library supplies.  One rule object serves one
// run of the chain, on either side, and carries the running claim.  A rule has
//     s                                 the statement: s.n variables, s.n_bind bound elements
//     TOP, MAX_FINALS, CHALLENGES       the top values, the most finals of a layer, and the challenges squeezed before a layer's
//                                       sumcheck, the last of which is that sumcheck's seed (product: seed; fraction: lambda, seed)
//     layer_statement(d), layer_at(d), layer_bytes(d), finals(d)
//                                       layer d's pks statement, where its proof starts, its length, and how many finals end it
//     start(top, rho), expected(ch), step(d, finals, ch, rho)
//                                       the claim from the top values, the sum layer d's sumcheck must state, the claim after layer d
//   verify_chain only:
//     check_top(top, result), check_finals(d, finals, ch, result)
//                                       the checks on the top values and on layer d's finals beyond its sumcheck's own; false: the
//                                       failed check's verdict (pk::verdict) is in *result
//   prove_chain only:
//     tables(d, ch, out)                the device tables of layer d's sumcheck into out[], after whatever launch makes them (on the
//                                       null stream, no synchronise: pks_prove's own launches follow there); != 0: the failure's code,
//                                       its reason already in the prover
//
// Also here: the frame a prover of such a chain holds and its creation.  Host only; of other libraries it calls what provekit_hip.h and
// provekit_sumcheck.h declare, and the prover's calls only in templates a prover instantiates: a verifier links none of them.
#pragma once
#include <memory>

#include "../argument.hpp"
#include "../prover_transcript.hpp"

namespace pk::gkr {

// The limits the frame and the two walks size their arrays by; each library asserts that its own are these.
constexpr unsigned MAX_VARS = 28, MAX_BIND = 16;

// ---- the prover's frame ----------------------------------------------------------------------------------------------------------

// What every prover of a chain holds next to its own arena, top values and profile.  EVENTS: the events it records on the null stream.
template <unsigned EVENTS>
struct ProverFrame {
    pk_ctx* ctx = nullptr;
    std::string pattern, err;
    pks_prover* layer[MAX_VARS] = {};  // layer[d], 1 <= d < n
    unsigned grid = 0;    // the workgroups of the library's kernels; 0: the rule.  No bit of a result depends on it
    unsigned layers = 0;  // layers per launch, 1 .. 3; 0: the library's value.  No bit of a result depends on it
    hipEvent_t ev[EVENTS] = {};

    ProverFrame() = default;
    ProverFrame(const ProverFrame&) = delete;
    ProverFrame& operator=(const ProverFrame&) = delete;
    // gives back the pks provers, the events and the arena, so a creation that stops half way leaks nothing; rc: the first failure's code
    int give_back(uint64_t*& arena) {
        int rc = PK_OK;
        for (pks_prover*& s : layer) {
            if (s)
                if (int r = pks_prover_destroy(s)) rc = rc ? rc : r;
            s = nullptr;
        }
        for (hipEvent_t& e : ev) {
            if (e) (void)hipEventDestroy(e);
            e = nullptr;
        }
        if (arena)
            if (int r = pk_free(ctx, arena)) rc = rc ? rc : r;
        arena = nullptr;
        return rc;
    }
};

// The common part of a prover's creation: the arena, the events and the pks provers of layers 1 .. n - 1.  `arena` is the prover's own
// member, so that what a failure leaves behind is given back with the prover; the reason of a failure goes to `slot`.
template <unsigned EVENTS, class LayerStatement>
int make_frame(ProverFrame<EVENTS>& p, pk_ctx* ctx, size_t arena_bytes, uint64_t*& arena, unsigned n, LayerStatement&& layer_statement, std::string& slot) {
    auto stop = [&](int rc, const std::string& reason) { return slot = reason, rc; };
    p.ctx = ctx;
    void* base = nullptr;
    if (int rc = pk_malloc(ctx, arena_bytes, &base)) return stop(rc, "pk_malloc of the arena failed");
    arena = (uint64_t*)base;
    for (hipEvent_t& e : p.ev)
        if (hipEventCreate(&e) != hipSuccess) return stop(PK_ERR_HIP, "hipEventCreate failed");
    for (unsigned d = 1; d < n; d++) {
        const pks_statement ps = layer_statement(d);
        if (int rc = pks_prover_create(ctx, &ps, &p.layer[d])) return stop(rc, std::string("pks_prover_create failed: ") + pks_create_error());
    }
    return PK_OK;
}

// ---- the prover's side -----------------------------------------------------------------------------------------------------------

// The protocol on the prover's tree as it stands: the outer transcript and the n - 1 pks proofs, into proof_out (rule.layer_at(n)
// bytes).  top: the rule's TOP top values; point_out: n elements or NULL.  The claim the chain ends on is in the rule.  p->prof.layer_ms[d]
// is layer d's pks_prove in host time.
template <class Prover, class Rule>
int prove_chain(Prover* p, Rule& rule, const fe* top, const uint64_t* bind, uint8_t* proof_out, uint64_t* point_out) {
    const unsigned n = rule.s.n;
    Transcript tr(p->pattern);
    for (unsigned i = 0; i < rule.s.n_bind; i++) tr.add_scalar(h_load(bind + 4 * i));
    tr.add_scalars(top, Rule::TOP);
    for (unsigned i = 0; i < Rule::TOP; i++) {
        const fe canon = h_to_canon(top[i]);
        memcpy(proof_out + 32 * i, canon.v, 32);
    }
    fe rho = tr.challenge_scalar();
    fe z[MAX_VARS], r[MAX_VARS], ch[Rule::CHALLENGES], finals[Rule::MAX_FINALS];
    rule.start(top, rho);
    z[0] = rho;
    for (unsigned d = 1; d < n; d++) {
        tr.challenge_scalars(ch, Rule::CHALLENGES);
        const fe& seed = ch[Rule::CHALLENGES - 1];
        const uint64_t* tables[Rule::MAX_FINALS];
        if (int rc = rule.tables(d, ch, tables)) return rc;
        size_t part = 0;
        const auto t0 = std::chrono::steady_clock::now();
        if (int rc = pks_prove(p->layer[d], tables, (const uint64_t*)z, (const uint64_t*)seed.v, proof_out + rule.layer_at(d), rule.layer_bytes(d), &part,
                               (uint64_t*)r, (uint64_t*)finals))
            return fail(p, rc, "layer " + std::to_string(d) + "'s sumcheck failed: " + pks_last_error(p->layer[d]));
        p->prof.layer_ms[d] = host_ms_since(t0);
        tr.add_scalars(finals, rule.finals(d));
        rho = tr.challenge_scalar();
        rule.step(d, finals, ch, rho);
        for (unsigned i = 0; i < d; i++) z[i + 1] = r[i];
        z[0] = rho;
    }
    if (!tr.finished()) return fail(p, PK_ERR_IO_PATTERN, "the transcript left its pattern: " + tr.violation());
    if (point_out) memcpy(point_out, z, 32 * (size_t)n);
    return PK_OK;
}

// ---- the verifier's side ---------------------------------------------------------------------------------------------------------

// One proof of exactly rule.layer_at(n) bytes against a parsed pattern.  PK_OK: the verdict is in *result, its offset in bytes of this
// proof, `layer` what it is about (0: the outer transcript or the top); accepted: point[0 .. n) is written and the claim the chain ends
// on is in the rule.  Another code: pks_verify refused, its reason in `slot`.
template <class Rule>
int verify_chain(Rule& rule, const pkv::Statement& st, const uint64_t* bind, const uint8_t* proof, fe* point, unsigned& layer, pkv_result* result,
                 std::string& slot) {
    const unsigned n = rule.s.n;
    constexpr size_t TOP_BYTES = 32 * (size_t)Rule::TOP;
    layer = 0;
    // the outer transcript reads one string: bind | top | the finals of every layer, which sit at the end of that layer's proof
    std::vector<uint8_t> bytes;
    bytes.reserve(32 * ((size_t)rule.s.n_bind + (size_t)Rule::MAX_FINALS * n));
    put_canonical(bytes, bind, rule.s.n_bind);
    const size_t prefix = bytes.size();
    bytes.insert(bytes.end(), proof, proof + TOP_BYTES);
    for (unsigned d = 1; d < n; d++) {
        const size_t end = rule.layer_at(d) + rule.layer_bytes(d);
        bytes.insert(bytes.end(), proof + end - 32 * (size_t)rule.finals(d), proof + end);
    }

    pkv::Verdict v;
    pkv::Arthur A(st, bytes.data(), bytes.size(), v);
    // an outer failure: inside top its own place, later the end of the layer whose finals were being absorbed
    auto outer_failed = [&](size_t proof_at) {
        if (!v.failed) A.fail(PKV_CHECK_TRANSCRIPT_SHORT, "the walk stopped without a verdict");
        v.offset = v.offset > prefix && v.offset <= prefix + TOP_BYTES ? v.offset - prefix : proof_at;
        pkv::to_result(v, result);
        layer = 0;
        return PK_OK;
    };
    fe scratch[MAX_BIND], top[Rule::TOP], rho, ch[Rule::CHALLENGES], finals[Rule::MAX_FINALS];
    if ((rule.s.n_bind && !A.next_scalars(rule.s.n_bind, scratch)) || !A.next_scalars(Rule::TOP, top)) return outer_failed(0);
    if (!rule.check_top(top, result)) return PK_OK;
    if (!A.challenge_scalars(1, &rho)) return outer_failed(TOP_BYTES);
    fe z[MAX_VARS], r[MAX_VARS];
    rule.start(top, rho);
    z[0] = rho;
    for (unsigned d = 1; d < n; d++) {
        const size_t at = rule.layer_at(d), end = at + rule.layer_bytes(d);
        for (fe& c : ch)
            if (!A.challenge_scalars(1, &c)) return outer_failed(at);
        const fe& seed = ch[Rule::CHALLENGES - 1];
        const pks_statement ps = rule.layer_statement(d);
        const fe sum = rule.expected(ch);
        const int rc = pks_verify(&ps, nullptr, 0, (const uint64_t*)z, (const uint64_t*)seed.v, (const uint64_t*)sum.v, proof + at, rule.layer_bytes(d), (uint64_t*)r,
                                  (uint64_t*)finals, result);
        if (rc) return slot = pks_create_error(), rc;
        result->offset += at;
        layer = d;
        if (!result->accepted) return PK_OK;
        if (!rule.check_finals(d, finals, ch, result)) return PK_OK;
        layer = 0;
        fe again[Rule::MAX_FINALS];  // the same bytes pks_verify took: canonical
        if (!A.next_scalars(rule.finals(d), again) || !A.challenge_scalars(1, &rho)) return outer_failed(end);
        rule.step(d, finals, ch, rho);
        for (unsigned i = 0; i < d; i++) z[i + 1] = r[i];
        z[0] = rho;
    }
    if (!A.done()) {
        A.fail(PKV_CHECK_IO_PATTERN, "declared operations left after the outer transcript");
        return outer_failed(rule.layer_at(n));
    }
    verdict(result, PKV_CHECK_NONE, rule.layer_at(n), "");
    for (unsigned i = 0; i < n; i++) point[i] = z[i];
    return PK_OK;
}

}  // namespace pk::gkr
