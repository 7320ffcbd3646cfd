// nrtr_joint.h - joint CTC / attention decoding (ccd_nrtr_joint_begin, ccd_nrtr_beam_step_joint): the beam over the NRTR attention
// decoder of nrtr_beam.h, every candidate rescored with the CTC PREFIX probability an auxiliary CTC head gives it (Hori, Watanabe,
// Hershey 2017).  tests/nrtr_joint_np.py restates the semantics in numpy and is the specification:
//   CTC side   frames [Tc, Cc] of a sample, lp = their fp64 log-probabilities (beam_wave_log_probs per frame), blank = class 0;
//              decoder class c != end_idx is CTC class k = c + class_offset.
//   a slot     carries, beside nrtr_beam.h's sequence / score / state, its attention score A (the plain beam's score) and the prefix
//              state rn[Tc], rb[Tc]: the log-probability that the frames 0..t spell exactly the slot's prefix g and end in a non-blank
//              / in a blank.  Root: rn = -inf, rb[t] = lp[0, 0] + .. + lp[t, 0].
//   extension  of g (last CTC class `last`) by k:  n[0] = lp[0, k] if g is empty else -inf, b[0] = -inf,
//              phi[t] = rb[t - 1] if k == last else lae(rn[t - 1], rb[t - 1]),
//              n[t] = lae(n[t - 1], phi[t]) + lp[t, k],  b[t] = lae(n[t - 1], b[t - 1]) + lp[t, 0];
//              psi(g.k) = log sum_t exp(phi[t] + lp[t, k]) (phi[0] = 0 for the empty g, -inf otherwise): the CTC output STARTS with g.k.
//              full(g) = lae(rn[Tc - 1], rb[Tc - 1]): the CTC output IS g.
//   candidates live slot r: (r, c), c != end_idx: S = (1 - w) (A_r + la[c]) + w psi(g_r.k); (r, end_idx): S = (1 - w) (A_r + la[end_idx]) + w
//              full(g_r); la = log_softmax(logits[r]).  It exists iff its attention part is finite and (w == 0 or its CTC part > -inf);
//              a class with k >= Cc has no CTC part.  At w == 0 S is the attention part itself - the bits of the plain beam.
//              A finished slot gives (r, end_idx) with S and A unchanged.  Selection, ties, tokens, parents, states: nrtr_beam.h's, on S.
//              A selected extension takes (n, b) as its prefix state, everything else keeps its parent's; an unused slot holds -inf.
//
// Step kernel: ONE WAVEFRONT PER SAMPLE, a kernel of its own beside nrtr_beam_step_kernel - NrtrJointWave is LDS the two instances
// there never allocate.  What the three share is called, not copied: nrtr_beam.h's nrtr_beam_stage, _carry, _select and _store, which
// hold the tie rule, the in-place update and the n-best lists.  Its own are the CTC parts of the phases below.  Lane l owns the
// classes l and l + 64, the positions l and l + 64 of a sequence, and frame l of a state.
//   1. nrtr_beam_stage, and the W parents' prefix states (lane t loads rn[t], rb[t] of every slot: W * 2 * Tc * 8 B <= 16 KB) and
//      attention scores: phase 4 overwrites `prefix` and `att` in place, after every load of the wave has landed in LDS.
//   2. per live slot: la by beam_wave_log_probs; lane t prepares phi[t] of the slot in both variants (k == last, k != last) in LDS;
//      then every lane runs the Tc frames for its two classes: phi[t] read at a wave-uniform address (both variants, a select picks),
//      lp[t, k] from the workspace, coalesced across the lanes.  Two passes (the maximum, then the sum of exp in ascending t): one
//      exp per term.  The joint score goes to the candidate table, the attention part to a second table of the same shape.  A slot
//      that is not live: nrtr_beam_carry, its attention score in the second table.
//   3. nrtr_beam_select over S; lane r then takes the attention part of its winner (i, c) from the second table, which stands.
//   4. lane r < W runs the Tc-step recursion of its new slot from the parent's staged state (or copies it) and stores it, with att;
//      nrtr_beam_store does the rest.
// Loops that shuffle run over W or have none inside (the frame loops are lane-local, trip count Tc); fp64 throughout.  LDS: 20.2 KB
// (nrtr_beam.h) + 16 KB attention parts + 16 KB staged states + 1.2 KB = 53.6 KB.
#pragma once

#include "nrtr_beam.h"

namespace ccd {

constexpr int NRTR_JOINT_MAX_T = 64;                               // frames of the CTC head (a lane per frame)

struct NrtrJointWave {
    ctc_real attc[NRTR_MAX_BEAM][NRTR_MAX_C];                      // the attention part of candidate (r, c)
    ctc_real pre[NRTR_MAX_BEAM][2][NRTR_JOINT_MAX_T];              // rn, rb of the old slots
    ctc_real att[NRTR_MAX_BEAM];
    ctc_real phi[2][NRTR_JOINT_MAX_T];                             // of the slot at hand: [0] k != last, [1] k == last
};
static_assert(sizeof(NrtrJointWave) == 33920, "with NrtrBeamWave: 54 592 B of LDS, the layout is fixed");

struct NrtrJoint {
    const ctc_real* lp;                                            // fp64 [B, Tc, Cc]: ccd_nrtr_joint_begin's workspace
    int Tc, Cc, class_offset;
    ctc_real w;
    ctc_real* prefix;                                              // fp64 [B, W, 2, Tc], in and out
    ctc_real* att;                                                 // fp64 [B, W], in and out
    float* att_scores;                                             // fp32 [B, W], written with the paths
};

// grid = B, block = 64.  frames fp32: frame t of sample b at frames + b * sample_stride + t * step_stride, Cc dense classes.  Writes
// lp [B, Tc, Cc] and the root state into the W slots of prefix [B, W, 2, Tc].  The launcher has checked 1 <= Tc <= 64, 1 <= Cc <= 128,
// 1 <= W <= 16.
__global__ __launch_bounds__(64) void nrtr_joint_begin_kernel(const float* __restrict__ frames, long sample_stride, long step_stride, int Tc,
                                                              int Cc, int normalized, int W, ctc_real* __restrict__ lp,
                                                              ctc_real* __restrict__ prefix) {
    __shared__ ctc_real row[NRTR_MAX_C];
    __shared__ ctc_real root[NRTR_JOINT_MAX_T];
    const int lane = lane_id(), b = blockIdx.x;
    const int c0 = lane, c1 = lane + 64;
    const bool has0 = c0 < Cc, has1 = c1 < Cc;
    ctc_real blank = 0;                                                    // lp[0, 0] + .. + lp[t, 0], ascending
    for (int t = 0; t < Tc; ++t) {
        const float* const x = frames + (long)b * sample_stride + (long)t * step_stride;
        const CtcReal2 v = beam_wave_log_probs(has0 ? x[c0] : 0.f, has1 ? x[c1] : 0.f, has0, has1, normalized != 0, row, Cc);
        ctc_real* const o = lp + ((long)b * Tc + t) * Cc;
        if (has0) o[c0] = v.c0;
        if (has1) o[c1] = v.c1;
        blank += shfl(v.c0, 0);
        if (lane == 0) root[t] = blank;
    }
    wave_lds_fence();
    if (lane < Tc) {
        const ctc_real rb = root[lane];
        for (int r = 0; r < W; ++r) {
            ctc_real* const p = prefix + ((long)b * W + r) * 2 * Tc;
            p[lane] = ctc_neg_inf();
            p[Tc + lane] = rb;
        }
    }
}

// log sum_t exp(phi[t] + lp[t * Cc]) over the Tc frames, phi = ph[1] where `same`, ph[0] elsewhere (read at wave-uniform addresses).
// Lane-local; -inf when every term is.
__device__ __forceinline__ ctc_real nrtr_joint_psi(const ctc_real (*ph)[NRTR_JOINT_MAX_T], const ctc_real* __restrict__ lp, int Tc, int Cc,
                                                   bool same) {
    ctc_real mx = ctc_neg_inf();
    for (int t = 0; t < Tc; ++t) {
        const ctc_real a = ph[0][t], s = ph[1][t];
        const ctc_real x = (same ? s : a) + lp[(long)t * Cc];
        mx = x > mx ? x : mx;
    }
    if (mx == ctc_neg_inf()) return mx;
    ctc_real sum = 0;
    for (int t = 0; t < Tc; ++t) {
        const ctc_real a = ph[0][t], s = ph[1][t];
        const ctc_real x = (same ? s : a) + lp[(long)t * Cc];
        sum += ::exp(x - mx);
    }
    return mx + ::log(sum);
}

// grid = B, block = 64.  Everything nrtr_beam_step_kernel<false> takes, checked as there; j: 1 <= Tc <= 64, 1 <= Cc <= 128,
// class_offset in {0, 1}, 0 <= w <= 1.  att_scores comes with the paths.
__global__ __launch_bounds__(64) void nrtr_beam_step_joint_kernel(const float* __restrict__ logits, long ldl, int W, int C, int step,
                                                                  int end_idx, int pad_idx, long long* seq, int seq_len, ctc_real* score,
                                                                  int* state, int* __restrict__ parent, int* __restrict__ paths,
                                                                  int* __restrict__ lengths, float* __restrict__ hyp_scores, NrtrJoint j) {
    __shared__ NrtrBeamWave s;
    __shared__ NrtrJointWave jw;
    const int lane = lane_id(), b = blockIdx.x;
    const int c0 = lane, c1 = lane + 64;
    const bool has0 = c0 < C, has1 = c1 < C;
    const long row0 = (long)b * W;
    const float ninf = -__builtin_inff();
    const int Tc = j.Tc, Cc = j.Cc;
    const ctc_real w = j.w;
    const bool fuse = w > 0;                                               // wave-uniform
    const ctc_real* const lp = j.lp + (long)b * Tc * Cc;
    ctc_real* const prefix = j.prefix + row0 * 2 * Tc;

    // ---- 1. the old state
    nrtr_beam_stage(s, seq, seq_len, score, state, row0, W, step);
    if (lane < NRTR_MAX_BEAM) jw.att[lane] = lane < W ? j.att[row0 + lane] : ctc_neg_inf();
    if (lane < Tc) {
        for (int r = 0; r < W; ++r) {
            jw.pre[r][0][lane] = prefix[(long)r * 2 * Tc + lane];
            jw.pre[r][1][lane] = prefix[(long)r * 2 * Tc + Tc + lane];
        }
    }
    wave_lds_fence();

    // ---- 2. the candidates
    const int k0 = c0 + j.class_offset, k1 = c1 + j.class_offset;          // the lane's CTC classes
    const bool ctc0 = has0 && c0 != end_idx && k0 < Cc, ctc1 = has1 && c1 != end_idx && k1 < Cc;
    for (int r = 0; r < W; ++r) {
        const int st = s.state[r];                                         // wave-uniform
        const ctc_real sc = s.score[r], at = jw.att[r];
        if (st == NRTR_LIVE) {
            const float* const x = logits + (row0 + r) * ldl;
            const CtcReal2 la = beam_wave_log_probs(has0 ? x[c0] : ninf, has1 ? x[c1] : ninf, has0, has1, false, s.cand[r], C);
            const ctc_real a0 = at + la.c0, a1 = at + la.c1;               // the attention parts (-inf stays -inf)
            ctc_real s0 = a0, s1 = a1;
            if (fuse) {
                if (lane < Tc) {                                           // phi[t] of this slot, both variants
                    const bool first = lane == 0;
                    const ctc_real rn = first ? ctc_neg_inf() : jw.pre[r][0][lane - 1], rb = first ? ctc_neg_inf() : jw.pre[r][1][lane - 1];
                    const ctc_real start = step == 0 ? (ctc_real)0 : ctc_neg_inf();      // the empty prefix opens at frame 0
                    jw.phi[0][lane] = first ? start : ctc_lae(rn, rb);
                    jw.phi[1][lane] = first ? start : rb;
                }
                wave_lds_fence();
                const int last = step == 0 ? -1 : (int)s.tok[r][step] + j.class_offset;
                const ctc_real full = ctc_lae(jw.pre[r][0][Tc - 1], jw.pre[r][1][Tc - 1]);
                const ctc_real p0 = nrtr_joint_psi(jw.phi, lp + (ctc0 ? k0 : 0), Tc, Cc, k0 == last);
                ctc_real p1 = ctc_neg_inf();
                if (C > 64) p1 = nrtr_joint_psi(jw.phi, lp + (ctc1 ? k1 : 0), Tc, Cc, k1 == last);     // (wave-uniform)
                const ctc_real t0 = c0 == end_idx ? full : (ctc0 ? p0 : ctc_neg_inf());
                const ctc_real t1 = c1 == end_idx ? full : (ctc1 ? p1 : ctc_neg_inf());
                s0 = a0 > ctc_neg_inf() && t0 > ctc_neg_inf() ? (1 - w) * a0 + w * t0 : ctc_neg_inf();
                s1 = a1 > ctc_neg_inf() && t1 > ctc_neg_inf() ? (1 - w) * a1 + w * t1 : ctc_neg_inf();
                wave_lds_fence();                                          // (phi is rewritten for the next slot)
            }
            if (has0) {
                s.cand[r][c0] = s0;
                jw.attc[r][c0] = a0;
            }
            if (has1) {
                s.cand[r][c1] = s1;
                jw.attc[r][c1] = a1;
            }
        } else {
            nrtr_beam_carry(s.cand[r], st, sc, end_idx, C);
            if (has0) jw.attc[r][c0] = at;
            if (has1) jw.attc[r][c1] = at;
        }
    }
    wave_lds_fence();

    // ---- 3. the W best by S; the attention part of lane r's winner still stands in the second table
    const NrtrBeamPick pick = nrtr_beam_select(s, W, C, end_idx, pad_idx);
    const ctc_real new_att = pick.parent >= 0 ? jw.attc[pick.parent][pick.c] : ctc_neg_inf();

    // ---- 4. the new state, in place: the prefix states come from LDS, which holds every old one
    if (lane < W) {
        j.att[row0 + lane] = new_att;
        if (hyp_scores) j.att_scores[row0 + lane] = pick.state == NRTR_UNUSED ? ninf : (float)new_att;
        const int p = pick.parent < 0 ? 0 : pick.parent;
        const int k = pick.tok + j.class_offset;
        const bool extend = pick.state == NRTR_LIVE, keep = pick.state == NRTR_FINISHED;
        const bool known = extend && k < Cc;                               // (a class without a CTC class: -inf throughout)
        const bool same = step > 0 && k == (int)s.tok[p][step] + j.class_offset;
        const ctc_real* const lk = lp + (known ? k : 0);
        ctc_real* const o = prefix + (long)lane * 2 * Tc;
        ctc_real n = known && step == 0 ? lk[0] : ctc_neg_inf(), bl = ctc_neg_inf();
        for (int t = 0; t < Tc; ++t) {
            const ctc_real rn = jw.pre[p][0][t], rb = jw.pre[p][1][t];
            if (known && t > 0) {
                const ctc_real rn1 = jw.pre[p][0][t - 1], rb1 = jw.pre[p][1][t - 1];
                const ctc_real phi = same ? rb1 : ctc_lae(rn1, rb1);
                const ctc_real n_new = ctc_lae(n, phi) + lk[(long)t * Cc];
                bl = ctc_lae(n, bl) + lp[(long)t * Cc];
                n = n_new;
            }
            o[t] = keep ? rn : n;
            o[Tc + t] = keep ? rb : bl;
        }
    }
    nrtr_beam_store(s, pick, seq, seq_len, score, state, parent, paths, lengths, hyp_scores, row0, W, step, end_idx);
}

}  // namespace ccd
