// life_rule_lane.h -- the rule network of RULE_LANE: a rule held per lane (the batch
// kernels with per-field rules, life_batch_rules.h; DESIGN §4 "Per-field rules").
//
// rule32_total's generic branch tests two scalar masks with uniform branches, so no two
// lanes of a launch can differ in their rule.  Here the masks are per-lane values and the
// rule is a branch-free multiplexer tree of v_bitop3 over the four bits of the 9-cell
// total T = H3(r-2) + H3(r-1) + H3(r) = s0 + 2 x + 4 t2 + 8 t3 (0..9; an alive cell has
// n = T - 1 neighbours, a dead one n = T):
//   * ten leaves, one per value v of T: leaf_0 = B0 and leaf_v = alive ? S(v-1) : B(v) for
//     v = 1..9, with B(k) / S(k) the lane's birth / survive bit k spread over all 32 bits
//     (one v_bfe_i32 each, loop-invariant) and B(9) = 0;
//   * the leaf of T chosen by s0 (5 selects), x (2), t2 (1) and t3 (1).
// 9 + 9 selects on top of the 7 operations that form the bits of T, per plane and row.
// T = 10..15 cannot occur (t3 implies x = t2 = 0), and an alive cell has T >= 1, so
// leaf_0 needs no S term.  (A dead cell cannot meet T = 9 either; leaf_9 keeps its B term
// so that the network is bit n = T - alive of the selected mask for every triple of H3
// sums, which is what tests/test_rule_lane_logic.py checks from the immediates below.)
//
// A header of its own: nothing here is seen by the stencil kernels' translation units.
#pragma once
#include "life_stencil.h"

namespace gol {

namespace {

constexpr uint32_t kLaneT2 = 0x6A;    // (a & b) ^ c: bit 2 of T from p, k0, mj
constexpr uint32_t kLaneT3 = 0x80;    // a & b & c: bit 3 of T
constexpr uint32_t kLaneLeaf = 0xCA;  // alive ? S(v-1) : B(v)
constexpr uint32_t kLaneSel0 = 0xCA;  // s0 ? leaf_{2j+1} : leaf_{2j}
constexpr uint32_t kLaneSel1 = 0xCA;  // x ? .. : ..
constexpr uint32_t kLaneSel2 = 0xCA;  // t2 ? .. : ..
constexpr uint32_t kLaneSel3 = 0xCA;  // t3 ? (T = 8, 9) : (T = 0..7)

// bit k of m on all 32 bits (v_bfe_i32)
__device__ __forceinline__ uint32_t lane_spread(uint32_t m, int k)
{
    return (uint32_t)((int32_t)(m << (31 - k)) >> 31);
}

// One plane of one row: (as, ac), (bs, bc), (es, ec) the H3 sums of rows r-2, r-1, r,
// `alive` the cells of row r-1, birth / survive the lane's 9-bit masks.
__device__ __forceinline__ uint32_t rule32_lane(uint32_t as, uint32_t ac, uint32_t bs, uint32_t bc,
                                                uint32_t es, uint32_t ec, uint32_t alive,
                                                uint32_t birth, uint32_t survive)
{
    const uint32_t s0 = lop3<kXor3>(as, bs, es);
    const uint32_t k0 = lop3<kMaj>(as, bs, es);
    const uint32_t p = lop3<kXor3>(ac, bc, ec);
    const uint32_t mj = lop3<kMaj>(ac, bc, ec);
    const uint32_t x = p ^ k0;
    const uint32_t t2 = lop3<kLaneT2>(p, k0, mj);
    const uint32_t t3 = lop3<kLaneT3>(p, k0, mj);
    uint32_t leaf[10];
    leaf[0] = lane_spread(birth, 0);
#pragma unroll
    for (int v = 1; v <= 9; ++v)
        leaf[v] = lop3<kLaneLeaf>(alive, lane_spread(survive, v - 1),
                                  v <= 8 ? lane_spread(birth, v) : 0u);
    uint32_t m[5];
#pragma unroll
    for (int j = 0; j < 5; ++j) m[j] = lop3<kLaneSel0>(s0, leaf[2 * j + 1], leaf[2 * j]);
    const uint32_t lo = lop3<kLaneSel1>(x, m[1], m[0]);  // T = 0..3
    const uint32_t hi = lop3<kLaneSel1>(x, m[3], m[2]);  // T = 4..7
    const uint32_t low8 = lop3<kLaneSel2>(t2, hi, lo);
    return lop3<kLaneSel3>(t3, m[4], low8);
}

// stage_step_ends (life_stencil.h) for RULE_LANE: no pair form, the rule per lane.
template <int NP>
__device__ __forceinline__ Pl<NP> stage_step_lane(StageT<NP>& st, const Pl<NP>& x, const Ends& e,
                                                  uint32_t birth, uint32_t survive)
{
    Pl<NP> s3, c3, y;
#pragma unroll
    for (int k = 0; k < NP; ++k) {
        const uint32_t L = left_of(x, e, k), R = right_of(x, e, k);
        s3.v[k] = lop3<kXor3>(L, x.v[k], R);
        c3.v[k] = lop3<kMaj>(L, x.v[k], R);
        y.v[k] = rule32_lane(st.ps.v[k], st.pc.v[k], st.cs.v[k], st.cc.v[k], s3.v[k], c3.v[k],
                             st.al.v[k], birth, survive);
    }
    st.ps = st.cs;
    st.pc = st.cc;
    st.cs = s3;
    st.cc = c3;
    st.al = x;
    return y;
}

}  // namespace

}  // namespace gol
