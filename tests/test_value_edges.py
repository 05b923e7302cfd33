"""The edge-value cluster (tests/value_edges_util.py) on the CPU: the oracle against an arbitrary-precision
restatement of NodeResourcesFit, and the conditions on the inputs that keep the GPU tests over this cluster
(tests/test_gpu_value_edges.py) from becoming vacuous."""
import numpy as np
import pytest

from koordinator_amd import abi, synth
from tests import value_edges_util as ve


@pytest.mark.parametrize("profile", list(ve.PROFILES))
def test_oracle_fit_equals_integer_reference(profile):
    c = ve.edge_cluster()
    cfg, (_, codes, plugin) = ve.oracle_eval(profile)
    rcodes, rscores = ve.fit_reference(c, list(cfg.fit.resource_weights))
    fit_bits = np.uint16(0x1F)
    bad = np.argwhere((codes & fit_bits) != rcodes)
    assert not len(bad), f"filter codes differ first at (pod, node) {bad[0]}"
    bad = np.argwhere(plugin[:, :, abi.GS_PLUGIN_FIT] != rscores)
    assert not len(bad), f"Fit scores differ first at (pod, node) {bad[0]}: oracle " \
                         f"{plugin[bad[0][0], bad[0][1], abi.GS_PLUGIN_FIT]} reference {rscores[bad[0][0], bad[0][1]]}"


def test_division_estimate_needs_both_corrections():
    """At least 5% of the cluster's own Fit cpu / memory pairs leave the float32 estimate one too high, and at least
    5% one too low: the GPU parity tests over this cluster exercise both correction branches of pct_floor."""
    dec, inc = ve.fit_pair_branches(ve.edge_cluster())
    print(f"\nedge cluster: {100 * dec:.1f}% of the Fit pairs need --q, {100 * inc:.1f}% need ++q")
    assert dec >= 0.05 and inc >= 0.05, (dec, inc)
    # make_cluster's round values, for contrast: no pair needs either
    d0, i0 = ve.fit_pair_branches(synth.make_cluster(ve.N_NODES, 64, 41))
    print(f"round cluster: {100 * d0:.2f}% / {100 * i0:.2f}%")


@pytest.mark.parametrize("profile", list(ve.PROFILES))
def test_every_verdict_occurs(profile):
    _, (_, codes, plugin) = ve.oracle_eval(profile)
    for bit in (0x01, 0x02, 0x04, 0x08, 0x10, 0x20):
        assert (codes & bit).any(), f"no pair fails with filter bit {bit:#x}"
    fit = plugin[:, :, abi.GS_PLUGIN_FIT]
    assert (fit == 0).any() and (fit == 100).any(), (int(fit.min()), int(fit.max()))
    assert (codes == 0).mean() > 0.2, "too few feasible pairs"


def test_edge_groups_hold_their_values():
    """the groups the builder promises"""
    c = ve.edge_cluster()
    nd, mt, p = c.nodes, c.metrics, c.pods
    al, rq = nd["allocatable"], nd["requested"]
    assert al[:, 1].max() == ve.MAX_EXACT and (al[list(ve.AIM), 1] % 2 == 1).all()
    assert (al[list(ve.AIM), 0] % 1000 != 0).all() and (al[:, 0] == 1).any()
    for s in range(4):
        assert (al[:, s] == 0).any(), s
        assert (rq[:, s] > al[:, s]).any(), s
    assert (mt["node_usage"]["cpu_milli"] > al[:, 0]).any() and (mt["node_usage"]["memory"] > al[:, 1]).any()
    free = al - rq
    for s, req in ((0, ve.X_CPU), (1, ve.X_MEM), (2, ve.E_EPH), (3, ve.BE_CPU)):
        assert (free[:, s] == req).any() and (free[:, s] == req - 1).any(), s
    left = nd["allowed_pod_number"] - nd["pod_count"]
    assert (left == 1).sum() >= 3 and (left == 0).sum() >= 2
    kinds = {ve.pod_kind(i) for i in range(len(p))}
    assert kinds == set(ve.KINDS) | {"replica"}
    assert (p["limits"][:, 1] == ve.MAX_EXACT).any() and (p["requests"][:, 1] == ve.MAX_EXACT).any()


# ---------------------------------------------------------------------------------------------------------------------
# the scheduling scenario of the GPU tests, checked on the oracle alone

def test_schedule_scenario_happens_on_the_oracle():
    c = ve.edge_cluster()
    cfg, want, _ = ve.oracle_schedule()
    multi, last_slot, exhausted = ve.batch_scenarios(c, cfg, want)
    print(f"\n{len(multi)} (batch, node) with several pods, last slots taken {last_slot}, "
          f"{len(exhausted)} batch-cpu pods behind an exhausted node; placed {(want['node'] >= 0).sum()} of {len(want)}")
    assert multi and last_slot and exhausted
    landed = np.unique(want["node"][want["node"] >= 0])
    assert len(np.intersect1d(landed, list(ve.AIM))) >= 10, "the byte-granular rows are not the ones landed on"
