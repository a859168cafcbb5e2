// The policy layer of the prover: R::generate_proof over the gathered siblings of b entities -- which sub-proofs a policy asks for and
// where they live (policy_plan.inc), on which lanes their groups run (PolicyLanes: verify_policy_device, host_verify.inc, uses it too).

// parties of the sub-proofs of one group from the gathered paths: proof g = e * k + j (entity e, sub-proof j of the group) takes
// the siblings start + j * m ... of its entity; pad parties are (0, Scalar::one()) with commitment B_blinding
__global__ void k_gather_parties(size_t b, int height, int start, int count, int m, int k, const uint64_t* pv, const uint32_t* pr,
                                 const uint32_t* pC, const uint32_t* Bb_comp, uint64_t* vals, uint32_t* blind, uint32_t* Vc) {
    size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= b * (size_t)k * (size_t)m) return;
    const size_t g = t / m, e = g / k;
    const int jj = (int)(t - g * m), j = (int)(g - e * k);
    uint32_t r[8] = {1, 0, 0, 0, 0, 0, 0, 0}, c[8];
    uint64_t v = 0;
    if (jj < count) {
        size_t s = e * (size_t)height + (size_t)(start + j * m + jj);
        v = pv[s];
        ld8(r, pr + s * 8);
        ld8(c, pC + s * 8);
    } else {
        for (int i = 0; i < 8; i++) c[i] = Bb_comp[i];
    }
    vals[t] = v;
    st8(blind + t * 8, r);
    st8(Vc + t * 8, c);
}

static bool policy_grouping_on() { return !knob("DAPOL_NO_GROUP"); }      // prover and verifier alike (policy_plan.inc: group_policy_plan)

// The groups of one small call side by side: group gi runs on lane gi % 4 (dapol_ctx::aux; lane 0 is the context itself), behind
// everything queued on the context's stream before fork().  A lane's kernels read and write buffers of the call, so the call may
// not be left while a lane runs: unless close() has marked the normal end (the caller has waited for, or joined, every lane), the
// destructor waits for every lane it handed out.  Declare it AFTER the buffers the lanes use.
struct PolicyLanes {
    dapol_ctx* c;
    bool touched[4] = {false, false, false, false};
    bool closed = false;
    explicit PolicyLanes(dapol_ctx* c_) : c(c_) {}
    PolicyLanes(const PolicyLanes&) = delete;
    int32_t fork(hipStream_t st) { HIPCHK(hipEventRecord(c->ev_v[0], st)); return DAPOL_OK; }     // (an event that no other path of a policy call uses)
    int32_t take(size_t gi, dapol_ctx** lane) {
        const int i = (int)(gi % 4);
        if (int32_t rc = ctx_lane(c, i, lane)) return rc;
        touched[i] = true;
        if (*lane != c) HIPCHK(hipStreamWaitEvent((*lane)->stream, c->ev_v[0], 0));
        return DAPOL_OK;
    }
    void close() { closed = true; }
    ~PolicyLanes() {
        if (closed) return;
        for (int i = 1; i < 4; i++)
            if (touched[i]) { (void)hipStreamSynchronize(c->aux[i - 1]->stream); g_fork_guard_waits.fetch_add(1, std::memory_order_relaxed); }
        (void)hipStreamSynchronize(c->stream);              // (lane 0, and what the context's stream queued behind the lanes; not a side lane: not counted)
    }
};

// R::generate_proof (src/range/padding.rs:88-118, splitting.rs:100-129) for b proofs over H siblings each: pv / pr / pC
// are [b][H] device arrays of the siblings' values, blindings and commitments; one RNG stream (d_stream[e]) per proof
// runs across its sub-proofs.  d_range: [b][sum of the plan's proof words].
// A run of the plan's sub-proofs of EQUAL size (the individual proofs of the siblings beyond aggregation_factor -- padding.rs:104-112,
// splitting.rs:118-123 -- with the one-party part of an odd split before them) is ONE call of b * k proofs (RangeArgs::sub_k): same
// draws, same bytes, one pipeline of full launches instead of k part-filled ones (round 6; DAPOL_NO_GROUP=1 proves them one by one).
static int32_t prove_policy_device(dapol_ctx* ctx, const std::vector<SubProof>& plan, size_t b, int H, const uint64_t* pv, const uint32_t* pr,
                                   const uint32_t* pC, int n_bits, const uint32_t* d_seed, const uint64_t* d_stream, uint32_t* d_range,
                                   MsmTiming* tm, const uint32_t* d_tape = nullptr /* [b][tape_slots][16]: tape mode */, size_t tape_slots = 0,
                                   uint32_t seed_stride = 0 /* words between the rows' seeds in d_seed; 0: one seed for the call */) {
    hipStream_t st = ctx->stream;
    const PolicyGroups PG = group_policy_plan(plan, policy_grouping_on());
    const std::vector<PolicyGroup>& groups = PG.groups;
    const uint32_t* Bb_comp = ctx->gens_comp.p + (size_t)ctx->tv.row_Bb(0) * 8;
    // A SMALL call whose plan has several groups (splitting at aggregation 24 = a 16-party and an 8-party proof: one of the reference's
    // six `prove` cases, benches/dapol.rs:71-78; any plan with individual proofs) is a chain of latencies per group, and the groups are
    // independent statements: each runs on a lane of its own (dapol_ctx::aux -- own streams, events and scratch, the same tables),
    // queued without a host wait, and the call waits for all of them at the end.  Same bytes (the groups' draws and outputs are
    // disjoint).  DAPOL_NO_LANES=1: one after the other.  It pays well beyond the latency regime -- while one group's kernels cannot
    // fill the chip, another's run beside them: padding at aggregation 24, one call of 1 / 16 / 256 / 1,024 / 4,096 entities 9.5 / 11.8 /
    // 22.9 / 42.0 / 117.4 ms one after the other, 6.2 / 8.8 / 17.6 / 38.0 / 110.1 ms on lanes; 8,192: -3 %, 16,384: -1 %
    // (profiles/r6_lanes_midsize.txt) -- so up to 40,000 sub-proofs per call.
    size_t lanes_max = 40000;                                // most sub-proofs of a call whose groups take lanes (DAPOL_LANES_MAX)
    if (const char* e = knob("DAPOL_LANES_MAX")) { long long v = atoll(e); if (v >= 2) lanes_max = (size_t)v; }
    const bool on_lanes = groups.size() >= 2 && groups.size() <= 64 && b * PG.sum_proofs <= lanes_max && !tm && !knob("DAPOL_NO_LANES");
    const PolicyLayout L = policy_layout(PG, b, n_bits, !on_lanes);
    DevBuf<uint64_t> vals;
    DevBuf<uint32_t> blind, Vc;
    HIPCHK(vals.alloc(L.parties)); HIPCHK(blind.alloc(L.parties * 8)); HIPCHK(Vc.alloc(L.parties * 8));
    // group gi's parties, on the context's stream
    auto gather = [&](size_t gi) -> int32_t {
        const PolicyGroup& g = groups[gi];
        const size_t at = L.g[gi].party_off;
        hipLaunchKernelGGL(k_gather_parties, dim3(nblk(b * (size_t)g.k * (size_t)g.m, 256)), dim3(256), 0, st, b, H, g.start, g.count, g.m, g.k, pv, pr, pC,
                           Bb_comp, vals.p + at, blind.p + at * 8, Vc.p + at * 8);
        LAUNCH_CHECK();
        return DAPOL_OK;
    };
    // group gi's proofs on `lane`: the group's first slot inside every entity's row of draws, its first word inside every entity's blob
    auto prove = [&](size_t gi, dapol_ctx* lane, MsmTiming* t, PendingProve* pend) -> int32_t {
        const PolicyGroup& g = groups[gi];
        const PolicyLayout::Group& lg = L.g[gi];
        return range_prove_device(lane, n_bits, g.m, b * (size_t)g.k, vals.p + lg.party_off, blind.p + lg.party_off * 8, Vc.p + lg.party_off * 8, d_seed, d_stream,
                                  lg.slot_base, d_tape ? d_tape + lg.slot_base * 16 : nullptr, d_range + lg.word_off, t, tape_slots, (uint32_t)g.k, L.entity_words,
                                  pend, seed_stride);
    };
    int32_t rc = DAPOL_OK;
    if (!on_lanes) {                                         // one group after the other: each call returns after its kernels have drained
        for (size_t gi = 0; gi < groups.size(); gi++)
            if ((rc = gather(gi)) || (rc = prove(gi, ctx, tm, nullptr))) return rc;
        HIPCHK(hipStreamSynchronize(st));
        return DAPOL_OK;
    }
    PolicyLanes lanes(ctx);
    std::vector<PendingProve> pend(groups.size());           // (sized once: the queued copies of the flags point into it)
    for (size_t gi = 0; gi < groups.size(); gi++)
        if ((rc = gather(gi))) return rc;
    if ((rc = lanes.fork(st))) return rc;
    for (size_t gi = 0; gi < groups.size(); gi++) {          // (an early return: `lanes` waits for the groups in flight)
        if (gi == 2) FAULT_AFTER_FORK("policy_prove_lanes");    // (group 1 is in flight on a lane of its own)
        dapol_ctx* lane = nullptr;
        if ((rc = lanes.take(gi, &lane))) return rc;
        pend[gi].pinned_slot = (int)((gi / 4) % 16);
        if ((rc = prove(gi, lane, nullptr, &pend[gi]))) return rc;
    }
    for (auto& pnd : pend) { int32_t r2 = pnd.finish(); if (!rc) rc = r2; }     // every group's zero-challenge flag, behind its lane
    lanes.close();
    if (rc) return rc;
    HIPCHK(hipStreamSynchronize(st));
    return DAPOL_OK;
}
