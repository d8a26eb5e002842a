"""The elimination planner (dags_vae_search_amd/eliminate.py) and the numpy restatement of tests/eliminate_corpus.py, on the CPU:
plan invariants, and the restatement against brute-force enumeration of the joint in exact rationals (chain48: against
forward-backward in rationals) within the derived bound gamma_D, with no extra factor."""
import numpy as np
import pytest

from dags_vae_search_amd import _lib as dl
from dags_vae_search_amd import eliminate as el
from tests import eliminate_corpus as ec


def _spans(plan):
    """per step: (the output's arena span or None, the arena spans of its inputs)"""
    return [((s["offset"], s["cells"]) if s["x"] >= 0 else None, [(f["offset"], f["cells"]) for f in s["inputs"] if f["kind"] < 0])
            for s in plan.steps]


def _disjoint(a, b):
    return a[0] + a[1] <= b[0] or b[0] + b[1] <= a[0]


@pytest.mark.parametrize("name", ec.NETWORKS + ("isolated",))
def test_plan_invariants(name):
    net = ec.network(name)
    n = len(net.card)
    for keep in ec.KEEPS.get(name, ((), (0, 3))):
        plan = ec.plan_of(name, keep)
        assert sorted(plan.order) == [v for v in range(n) if v not in keep] and plan.steps[-1]["x"] == -1
        used = [f["kind"] for s in plan.steps for f in s["inputs"] if f["kind"] >= 0]
        assert sorted(used) == list(range(n))                                     # every table is consumed exactly once
        made = [id(s) for s in plan.steps[:-1]]
        eaten = [(f["offset"], f["cells"], f["depth"]) for s in plan.steps for f in s["inputs"] if f["kind"] < 0]
        assert len(eaten) == len(made) == len(plan.order)                         # every intermediate is consumed exactly once
        live = []
        for s, (out, ins) in zip(plan.steps, _spans(plan)):
            assert all(span in live for span in ins)
            if out is not None:
                assert all(_disjoint(out, span) for span in live), (name, keep)   # clear of its inputs and of everything live
                assert out[0] + out[1] <= plan.arena_cells
                live.append(out)
            for span in ins:
                live.remove(span)
            assert s["cells"] == int(np.prod([int(net.card[v]) for v in s["scope"]], dtype=np.int64)) if s["scope"] else s["cells"] == 1
        assert live == [] and plan.out_cells == int(np.prod([int(net.card[v]) for v in keep], dtype=np.int64)) if keep else plan.out_cells == 1
        assert plan.words.dtype == np.int32 and plan.words[0] == dl.ELIM_TAG and len(plan.words) <= dl.ELIM_MAX_WORDS


def test_chain48_eliminates_with_scopes_of_two_for_any_kept_variable():
    for t in range(48):
        plan = ec.plan_of("chain48", (t,))
        assert plan.width <= 2 + (0 < t < 47) and max(len(s["scope"]) for s in plan.steps) <= 2, t
        assert all(len(s["scope"]) + 1 <= 2 or t in s["scope"] for s in plan.steps[:-1]), t
    assert ec.plan_of("chain48", ()).width == 2


def test_asia_width_and_arena_are_what_the_planner_gave_when_this_was_written():
    plan = ec.plan_of("asia", ())
    assert (plan.order, plan.width, plan.max_step_cells, plan.arena_cells, plan.depth) == ([2, 0, 6, 1, 3, 4, 5, 7], 4, 8, 17, 11)
    assert len(plan.words) == 152


def test_band48_fits_and_the_dense_network_does_not():
    for keep in ec.KEEPS["band48"]:
        plan = ec.plan_of("band48", keep)
        print(f"band48 keep {keep}: width {plan.width}, largest step {plan.max_step_cells}, arena {plan.arena_cells} cells, "
              f"depth {plan.depth}, {len(plan.words)} words")
        assert plan.arena_cells <= dl.ELIM_MAX_CELLS and plan.max_step_cells <= dl.ELIM_MAX_CELLS
    net = ec.network("dense")
    with pytest.raises(ValueError, match=r"width \d+ needs a table of \d+ cells and an arena of \d+ cells") as e:
        el.plan_network(net.card, net.masks, ())
    print(e.value)


def test_order_and_keep_are_validated():
    net = ec.network("hand")
    for order in ([0, 1], [0, 1, 1], [0, 1, 3], [0, 1, 2, 2]):
        with pytest.raises(ValueError, match="permutation"):
            el.plan_network(net.card, net.masks, (), order=order)
    with pytest.raises(ValueError, match="permutation"):
        el.plan_network(net.card, net.masks, (2,), order=[0, 1, 2])
    with pytest.raises(ValueError, match="keep"):
        el.plan_network(net.card, net.masks, (3,))
    with pytest.raises(ValueError, match="cap is 3"):
        el.plan_network(net.card, net.masks, (), max_cells=3)
    a = el.plan_network(net.card, net.masks, (2,), order=[1, 0])
    assert a.order == [1, 0] and a.keep == (2,)


@pytest.mark.parametrize("name", ec.ENUMERABLE)
def test_restatement_against_enumeration_in_exact_rationals(name):
    """keep empty, each single target, one pair; seeded partial evidence and events, an empty allowed set and (hand, zeroone)
    evidence of probability zero"""
    net = ec.network(name)
    n = len(net.card)
    masks = ec.query_masks(name, 8, seed=17)
    if name == "hand":                                                            # wet without rain or sprinkler
        masks[5] = [1, 1, 2]
    if name == "zeroone":                                                         # a level of probability zero under its parent
        j = next(j for j in range(net.tables[3].shape[0]) if (net.tables[3][j] == 0.0).any())
        masks[5] = 0xFFFF
        masks[5, 2], masks[5, 3] = 1 << j, 1 << int(np.argmin(net.tables[3][j]))
    keeps = [()] + [(v,) for v in range(n)] + [(0, n - 1)]
    zero = 0
    for keep in keeps:
        _, z = ec.check_against_exact(name, ec.plan_of(name, keep), masks, lambda row, kp: ec.exact_cells(name, row, kp))
        zero += int((z == 0.0).sum())
    assert zero >= 2 * len(keeps)                                                 # the empty sets; the impossible evidence


def test_restatement_on_chain48_against_forward_backward_in_rationals():
    masks = ec.query_masks("chain48", 6, seed=19)
    for keep in ((), (0,), (17,), (47,)):
        ec.check_against_exact("chain48", ec.plan_of("chain48", keep), masks, ec.chain_exact)


def test_an_explicit_order_gives_the_same_distribution():
    masks = ec.query_masks("six", 5, seed=23)
    exact = lambda row, kp: ec.exact_cells("six", row, kp)
    for _, plan in ec.loop_shape_plans()[:4]:
        ec.check_against_exact("six", plan, masks, exact)


def test_companion_header_binding():
    assert len(dl.EXPORTS) == 64 and "dvs_bn_eliminate" not in dl.SIGNATURES and list(dl.EXT_SIGNATURES) == ["dvs_bn_eliminate"]
    assert dl.signature("dvs_bn_eliminate") is dl.EXT_SIGNATURES["dvs_bn_eliminate"] and dl.signature("dvs_bn_lw") is dl.SIGNATURES["dvs_bn_lw"]
    assert (dl.ELIM_MAX_CELLS, dl.ELIM_MAX_WORDS, dl.ABI_VERSION) == (16384, 4096, 202)
    with pytest.raises(KeyError):
        dl.signature("dvs_no_such_call")


def test_a_missing_companion_header_is_an_error_that_gives_its_path(tmp_path):
    path = str(tmp_path / "include" / "dvs_eliminate.h")
    with pytest.raises(RuntimeError, match="dvs_eliminate.h not found at") as e:
        dl._read_header(path)
    assert path in str(e.value)
