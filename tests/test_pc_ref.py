"""The references of tests/pc_corpus.py pinned on the CPU, without the library: closed forms of the p-value, a hand-computed
table, the two restatements of the statistics against each other, the d-separation oracle on the three-vertex patterns, the
test order of a level and the orientation step."""
import math

import mpmath
import numpy as np
import pytest

from tests import pc_corpus as pc


def test_gamma_q_closed_forms():
    for s in (0.0, 0.3, 2.0, 17.5, 400.0):
        assert abs(pc.gamma_q(2, s) - mpmath.exp(-mpmath.mpf(s) / 2)) < mpmath.mpf(10) ** -40
        assert abs(pc.gamma_q(1, s) - mpmath.erfc(mpmath.sqrt(mpmath.mpf(s) / 2))) < mpmath.mpf(10) ** -40
    assert pc.gamma_q(0, 3.0) == 1


def test_statistics_of_a_hand_table():
    # x, y binary, no conditioning: counts [[10, 20], [30, 40]]
    data = np.array([[0, 0]] * 10 + [[0, 1]] * 20 + [[1, 0]] * 30 + [[1, 1]] * 40, np.uint8)
    card = np.array([2, 2], np.uint8)
    n, rows, cols = 100, (30, 70), (40, 60)
    cells = {(0, 0): 10, (0, 1): 20, (1, 0): 30, (1, 1): 40}
    g2 = 2 * sum(c * math.log(c * n / (rows[i] * cols[k])) for (i, k), c in cells.items())
    x2 = sum((c - rows[i] * cols[k] / n) ** 2 / (rows[i] * cols[k] / n) for (i, k), c in cells.items())
    for typ, want in (("mi", g2), ("x2", x2), ("mi-adf", g2), ("x2-adf", x2)):
        stat, df, p = pc.data_test(data, card, 0, 1, 0, typ)
        assert abs(stat - want) < 1e-12 and df == 1 and abs(p - float(pc.gamma_q(1, stat))) < 1e-15


@pytest.mark.parametrize("typ", pc.TYPES)
def test_the_two_restatements_of_the_statistics_agree(typ):
    case = pc.ci_case("sixS1000")
    for t, (x, y, zs) in enumerate(case.tests):
        if t in case.refused:
            continue
        stat, df, T = pc.ci_reference("sixS1000", x, y, zs, typ)
        got, gdf, _ = pc.data_test(case.data, case.card, x, y, pc.mask_of(zs), typ)
        assert gdf == df and abs(got - float(stat)) <= 1e-12 * T, (typ, t)


def test_dsep_oracle_on_chain_fork_and_collider():
    chain, fork, collider = [0, 0b001, 0b010], [0b010, 0, 0b010], [0, 0b101, 0]         # 0 -> 1 -> 2; 0 <- 1 -> 2; 0 -> 1 <- 2
    for P in (chain, fork):
        ind = pc.dsep_oracle(P)
        assert not ind(0, 2, 0) and ind(0, 2, 0b010) and not ind(0, 1, 0) and not ind(0, 1, 0b100)
    ind = pc.dsep_oracle(collider)
    assert ind(0, 2, 0) and not ind(0, 2, 0b010)
    # a descendant of the collider opens the path as well: 0 -> 1 <- 2, 1 -> 3
    ind = pc.dsep_oracle([0, 0b101, 0, 0b010])
    assert ind(0, 2, 0) and not ind(0, 2, 0b1000) and ind(0, 3, 0b010)


def test_level_order_is_side_x_then_side_y_each_by_ascending_mask():
    adj = [0b1110, 0b1101, 0b1011, 0b0111]                          # the complete graph on four vertices
    pair_xy, offsets, tests = pc.ref_level(adj, 1)
    assert pair_xy[0] == [0, 1] and offsets[:2] == [0, 4]
    assert [m for _, _, m in tests[:4]] == [0b0100, 0b1000, 0b0100, 0b1000]
    assert [len(pc.ref_level(adj, level)[2]) for level in range(4)] == [6, 24, 12, 0]
    assert pc.ref_level([0b10, 0b01], 1, every_pair=True)[:2] == ([[0, 1]], [0, 0])


def test_orient_ref_collider_and_meek_r1():
    full = (1 << 48) - 1
    adj = [0b0100, 0b0100, 0b1011, 0b0100]                          # 0 - 2, 1 - 2, 2 - 3
    sep = np.full((4, 4), full, np.uint64)
    sep[0, 1] = sep[1, 0] = 0
    assert pc.orient_ref(adj, sep) == ([0, 0, 0b0011, 0b0100], 0, 0)
    assert pc.orient_ref(adj, np.full((4, 4), full, np.uint64)) == (adj, 0, 0)                 # no collider: nothing is directed


def test_pc_ref_with_the_oracle_recovers_the_skeleton_and_the_separating_sets():
    P = [0, 0, 0b0011, 0b0100]                                      # 0 -> 2 <- 1, 2 -> 3
    r = pc.pc_ref(4, pc.dsep_oracle(P))
    assert r.adj == [0b0100, 0b0100, 0b1011, 0b0100] and r.tests_per_level[0] == 6
    assert int(r.sepset[0, 1]) == 0 and int(r.sepset[0, 3]) == 0b0100 == int(r.sepset[3, 1])
    assert pc.orient_ref(r.adj, r.sepset)[0] == [0, 0, 0b0011, 0b0100]
