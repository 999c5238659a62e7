"""The one table, generator and stem plan behind the fourteen CViT variants
(weights.CVIT_FAMILY, variants.stem_plan), CPU side.

The table-driven ``param_specs`` / ``synthetic_state_dict`` against the layout
and checksums the four per-family generators gave before they were merged
(tests/golden/cvit_family_checksums.json, tools/make_family_checksums.py);
``stem_plan`` against the launches of four representative classes, written out;
what ``stem_features``' ``upto`` accepts.
"""
import numpy as np
import pytest

from fac_fake_amd import weights as W
from fac_fake_amd.variants import Step, VariantCViT, stem_plan, steps_upto, variant_class

REPBN8, REPBN3, DCONV, SMFA = (W.REPBN8_NAME, "cvit_GGCA_ADD_DEConv_RepBn3", W.DCONV_NAME, "cvit_GGCA_SMFA")


def test_the_registry_is_assembled_from_the_four_tables():
    assert W.FAMILY_NAMES == (REPBN8, *W.VARIANT_NAMES, DCONV, *W.OTHER_NAMES) and len(W.FAMILY_NAMES) == 14
    for name, entry in W.CVIT_FAMILY.items():
        assert set(entry) == {"layers", "ggca", "ff_norm", "deconv", "smfa"}, name
        assert all(len(l) == 8 and l[2] in ("conv", "deconv", "idw") for l in entry["layers"]), name
    assert all(W.CVIT_FAMILY[n] is W.VARIANTS[n] for n in W.VARIANT_NAMES)
    assert all(W.CVIT_FAMILY[n] is W.OTHER_VARIANTS[n] for n in W.OTHER_NAMES)
    assert W.CVIT_FAMILY[REPBN8]["layers"] is W.REPBN8_LAYERS
    assert [(i, k, ci, co, bn, p) for _s, i, k, ci, co, bn, _r, p in W.CVIT_FAMILY[DCONV]["layers"]] == W.DCONV_LAYERS


@pytest.mark.parametrize("name", W.FAMILY_NAMES)
def test_specs_and_synthetic_weights_are_what_the_four_generators_gave(golden, name):
    fixture = golden("cvit_family_checksums.json")
    assert list(fixture["classes"]) == list(W.FAMILY_NAMES)
    # [key, shape, sum, abs-sum] and, unless float32, the dtype, in the state_dict's order
    want = [fixture["tensors"][i] for i in fixture["classes"][name]]
    specs = W.param_specs(W.CVIT_FAMILY[name])
    assert [[k, list(s)] for k, s, _ in specs] == [r[:2] for r in want]
    sd = W.synthetic_state_dict(specs, 0)
    sums = W.state_dict_checksums(sd)
    got = [[k, list(v.shape), *sums[k]] + ([str(v.dtype)] if v.dtype != np.float32 else []) for k, v in sd.items()]
    assert got == want
    assert {r[4] for r in want if len(r) > 4} <= {"int64"} and any(len(r) > 4 for r in want)


def test_the_old_entry_points_are_the_table_driven_ones():
    assert W.repbn8_param_specs() == W.param_specs(W.CVIT_FAMILY[REPBN8])
    assert W.dconv_param_specs() == W.param_specs(W.CVIT_FAMILY[DCONV])
    assert W.variant_param_specs(REPBN3) == W.param_specs(W.VARIANTS[REPBN3])
    assert W.other_param_specs(SMFA, depth=1) == W.param_specs(W.OTHER_VARIANTS[SMFA], depth=1)
    for make, args in ((W.make_repbn8_state_dict, ()), (W.make_dconv_state_dict, ()),
                       (W.make_variant_state_dict, (REPBN3,)), (W.make_other_state_dict, (SMFA,))):
        name = args[0] if args else {W.make_repbn8_state_dict: REPBN8, W.make_dconv_state_dict: DCONV}[make]
        a, b = make(*args, 1, depth=1), W.make_family_state_dict(name, 1, depth=1)
        assert list(a) == list(b) and all(np.array_equal(a[k], b[k]) and a[k].dtype == b[k].dtype for k in a)
    with pytest.raises(KeyError):
        W.variant_param_specs(DCONV)
    with pytest.raises(KeyError):
        W.other_param_specs(REPBN3)


def _convs(rows):
    """Step("conv", ...) per (n, H, ci, co, pool[, relu[, extra label]])."""
    return [Step("conv", (r[0], *r[6:]), r[1], r[2], r[3], r[4], r[5] if len(r) > 5 else True) for r in rows]


def test_plan_repbn8():
    plan = stem_plan(W.CVIT_FAMILY[REPBN8])
    assert plan[0] == Step("stem224", (3,), 224, 3, 32, True, True)
    assert plan[1:-1] == _convs([
        (4, 112, 32, 64, False), (5, 112, 64, 64, False), (6, 112, 64, 64, True),
        (7, 56, 64, 128, False), (8, 56, 128, 128, False), (9, 56, 128, 128, False, False),   # features1.26: no ReLU
        (10, 56, 128, 128, True),
        (11, 28, 128, 256, False), (12, 28, 256, 256, False), (13, 28, 256, 256, False),
        (14, 28, 256, 256, True, True, "features1"),
        (15, 14, 256, 512, False), (16, 14, 512, 512, False), (17, 14, 512, 512, False), (18, 14, 512, 512, True)])
    assert plan[-1] == Step("ggca", ("ggca",), 7, 512, 512, op="mul") and len(plan) == 17
    # H and pool as the table has them
    H = 112
    for s, l in zip(plan[1:-1], W.REPBN8_LAYERS[3:]):
        assert (s.H, s.ci, s.co, s.relu, s.pool) == (H, *l[3:5], *l[6:])
        H //= 2 if l[7] else 1


def test_plan_repbn3_has_its_ggca_on_the_56x56_map():
    plan = stem_plan(W.CVIT_FAMILY[REPBN3])
    assert [s.kind for s in plan] == ["stem224"] + ["conv"] * 3 + ["ggca"] + ["conv"] * 11
    assert plan[1:4] == _convs([(4, 112, 32, 64, False), (5, 112, 64, 64, False),
                                (6, 112, 64, 64, True, True, "features1")])
    assert plan[4] == Step("ggca", ("ggca",), 56, 64, 64, op="add")
    assert plan[5] == _convs([(7, 56, 64, 128, False)])[0] and plan[-1] == _convs([(17, 14, 512, 512, True)])[0]


def test_plan_dconv_starts_from_the_packed_input():
    plan = stem_plan(W.CVIT_FAMILY[DCONV])
    assert plan[0] == Step("pack32", (), 224, 3, 32)
    assert "".join(s.kind[0] for s in plan[1:-1]) == W.DCONV_KINDS.replace(" ", "") and len(plan) == 19
    assert plan[1] == Step("conv", (1,), 224, 32, 32, False, True)          # on the 32-channel packed input
    assert plan[2] == Step("idw", (2,), 224, 32, 32, False, True)
    assert plan[3] == Step("idw", (3,), 224, 32, 32, True, True)
    assert plan[4] == Step("conv", (4,), 112, 32, 64, False, True)
    H = 224
    for n, (s, (_i, kind, ci, co, _bn, pool)) in enumerate(zip(plan[1:-1], W.DCONV_LAYERS), 1):
        assert (s.kind, s.H, s.co, s.pool, s.relu) == (kind, H, co, pool, True) and s.labels[0] == n
        assert s.ci == (co if kind == "idw" else max(ci, 32))
        H //= 2 if pool else 1
    assert plan[-2].labels == (17, "features1")
    assert plan[-1] == Step("ggca", ("ggca",), 7, 512, 512, op="add")


def test_plan_smfa_block_sits_between_features1_and_features2():
    plan = stem_plan(W.CVIT_FAMILY[SMFA])
    # features1 is 13 plain convs: the fused three, then ten launches
    assert [s.kind for s in plan] == ["stem224"] + ["conv"] * 10 + ["smfa"] + ["conv"] * 4 + ["ggca"]
    assert plan[10] == Step("conv", (13, "features1"), 28, 256, 256, True, True)
    assert plan[11] == Step("smfa", ("smfa",), 14, 256, 256)
    assert plan[12] == Step("conv", (14,), 14, 256, 512, False, True)
    assert plan[-1] == Step("ggca", ("ggca",), 7, 512, 512, op="add")


@pytest.mark.parametrize("name", W.FAMILY_NAMES)
def test_plan_covers_every_layer_once(name):
    entry = W.CVIT_FAMILY[name]
    plan = stem_plan(entry)
    kinds = [s.kind for s in plan]
    assert kinds[0] in ("stem224", "pack32") and not {"stem224", "pack32"} & set(kinds[1:])
    fused = kinds[0] == "stem224"
    assert fused == all(l[2] != "idw" for l in entry["layers"][:3])
    assert kinds.count("conv") + kinds.count("idw") + 3 * fused == len(entry["layers"])
    assert kinds.count("ggca") == (entry["ggca"] is not None) and kinds.count("smfa") == (entry["smfa"] is not None)
    ints = [l for s in plan for l in s.labels if isinstance(l, int)]
    assert ints == list(range(3 if fused else 1, len(entry["layers"]) + 1))
    assert plan[-1].co == 512 and (plan[-1].H // 2 if plan[-1].pool else plan[-1].H) == 7
    if entry["ggca"] is not None:
        g = plan[kinds.index("ggca")]
        assert (g.co, g.H) == entry["ggca"][1][:2] and g.op == entry["ggca"][2]
        before = plan[kinds.index("ggca") - 1]
        assert before.co == g.co and (before.H // 2 if before.pool else before.H) == g.H


def test_int_upto_counts_table_layers_and_is_refused_inside_the_fused_block():
    for name in (REPBN8, REPBN3, SMFA, "cvit_DEConv"):
        plan, last = stem_plan(W.CVIT_FAMILY[name]), len(W.CVIT_FAMILY[name]["layers"])
        assert steps_upto(plan, None) == len(plan)
        for n in (0, 1, 2, last + 1, "nope"):
            with pytest.raises(ValueError):
                steps_upto(plan, n)
        assert steps_upto(plan, 3) == 1 and steps_upto(plan, 4) == 2          # the fused block, one conv more
        assert plan[steps_upto(plan, last) - 1].labels[0] == last and plan[steps_upto(plan, last) - 1].kind == "conv"
        assert "features1" in plan[steps_upto(plan, "features1") - 1].labels
    d = stem_plan(W.CVIT_FAMILY[DCONV])
    assert [steps_upto(d, n) for n in (1, 2, 3, 17, "features1", "ggca")] == [2, 3, 4, 18, 18, 19]
    assert d[steps_upto(d, 3) - 1] == Step("idw", (3,), 224, 32, 32, True, True)   # tests/test_dconv_gpu.py's stop
    for n in (0, 18, "smfa"):
        with pytest.raises(ValueError):
            steps_upto(d, n)
    with pytest.raises(ValueError):
        steps_upto(stem_plan(W.CVIT_FAMILY["cvit_DEConv"]), "ggca")              # the class has no GGCA
    smfa = stem_plan(W.CVIT_FAMILY[SMFA])
    assert [steps_upto(smfa, n) for n in ("features1", "smfa", "ggca")] == [11, 12, 17]
    assert steps_upto(stem_plan(W.CVIT_FAMILY[REPBN3]), "ggca") == 5


def test_one_factory_serves_every_name():
    from fac_fake_amd import dconv, other, repbn8, variants
    assert variant_class(REPBN8) is repbn8.CViT and variant_class(DCONV) is dconv.CViT
    assert variant_class(SMFA) is other.other_class(SMFA) and issubclass(variant_class(SMFA), other.OtherCViT)
    assert all(issubclass(variant_class(n), VariantCViT) and variant_class(n).variant == n for n in W.FAMILY_NAMES)
    assert len({variant_class(n) for n in W.FAMILY_NAMES}) == 14
    for bad in (lambda: variant_class("cvit"), lambda: other.other_class(REPBN3), lambda: variants.CViT(SMFA)):
        with pytest.raises(KeyError):
            bad()
    with pytest.raises(TypeError):
        VariantCViT()
