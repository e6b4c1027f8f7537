"""The BLS12-381 pairing, the part that exists so far and needs no GPU: the model that defines it (tools/bls12_381_pairing_model.py) recomputes fixture pairings
from the definition, is bilinear in both arguments, maps the tower to the polynomial form and back, and regenerates the committed fixture byte for byte."""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import bls12_381_pairing_model as model      # noqa: E402

g1, g2 = model.g1, model.g2
P, R = model.P, model.R


@pytest.fixture(scope="module")
def fx():
    return json.load(open(model.FIXTURE))


def pair_of(rec):
    return g1.decode96(bytes.fromhex(rec["g1"])), g2.decode192(bytes.fromhex(rec["g2"]))


# ---- the model and the fixture
def test_the_model_recomputes_two_fixture_pairings_and_is_bilinear_on_one_pair(fx):
    gt = model.gt_decode(bytes.fromhex(fx["generators"]))
    assert gt != model.ONE and model.f12_pow(gt, R) == model.ONE
    for rec in fx["pairings"][:2]:
        p, q = pair_of(rec)
        assert model.gt_encode(model.pairing(p, q)).hex() == rec["gt"]
    p, q = pair_of(fx["pairings"][1])
    e = model.gt_decode(bytes.fromhex(fx["pairings"][1]["gt"]))
    assert model.pairing(g1.mul(5, p), q) == model.f12_pow(e, 5) == model.pairing(p, g2.mul(5, q))
    assert model.pairing(None, q) == model.ONE == model.pairing(p, None)
    kinds = {(pair_of(r)[0] is None, pair_of(r)[1] is None) for r in fx["pairings"]}
    assert kinds == {(False, False), (True, False), (False, True), (True, True)}
    one = bytes(47) + b"\x01" + bytes(528)
    assert all(bytes.fromhex(r["gt"]) == one for r in fx["pairings"] if None in pair_of(r)) and model.gt_encode(model.ONE) == one


def test_the_fixture_regenerates_byte_for_byte_and_stays_small(fx):
    stored = open(model.FIXTURE).read()
    assert stored == model.fixture_text()
    assert len(stored) < 128 * 1024 and len(fx["pairings"]) >= 6
    ops = [tuple(int(v, 16) for v in t) for t in fx["tower_operands"]]
    assert (0,) * 12 in ops and (1,) + (0,) * 11 in ops and (P - 1,) * 12 in ops
    for c in fx["cyclotomic"]:
        a = model.to_poly(tuple(int(v, 16) for v in c))
        assert model.f12_mul(a, model.f12_conj(a)) == model.ONE
    t = tuple(range(1, 13))
    assert model.to_tower(model.to_poly(t)) == t and model.tower_mul((0, 1) + (0,) * 10, (0, 1) + (0,) * 10) == (P - 1,) + (0,) * 11      # u^2 = -1 through the map
    a = model.to_poly(ops[-1])
    assert model.f12_mul(a, model.f12_inv(a)) == model.ONE and model.f12_frobenius(a, 6) == model.f12_conj(a)
    assert fx["malformed_g1"] and fx["malformed_g2"] and fx["off_subgroup_g1"] and fx["off_subgroup_g2"]
