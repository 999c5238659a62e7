"""Pin the state_dict layout and the synthetic weights of the fourteen CViT
variants (RepBn8, weights.VARIANTS, cvit_GGCA_ADD_DConv, weights.OTHER_VARIANTS).

Writes tests/golden/cvit_family_checksums.json, the seed-0 synthetic state_dict
of each class: "tensors", every distinct ``[key, shape, sum, abs-sum]`` (the
float64 sums of ``weights.state_dict_checksums``; a fifth item names a dtype
other than float32), and "classes", per reference file name the ordered indices
into it (most keys are shared between classes).  It goes through the four
per-family generators' public names, so it runs unchanged on any revision that
has them; tests/test_cvit_family.py holds the one table-driven generator
against the file.
"""
from __future__ import annotations

import json
import sys
from pathlib import Path

sys.dont_write_bytecode = True
REPO = Path(__file__).resolve().parents[1]
OUT = REPO / "tests" / "golden" / "cvit_family_checksums.json"
sys.path.insert(0, str(REPO))

from fac_fake_amd import weights as W  # noqa: E402

SEED = 0


def generators():
    """name -> the family generator's call, in the order RepBn8, VARIANTS, DConv, OTHER_VARIANTS."""
    gens = {"cvit_GGCA_ADD_DEConv_RepBn8": lambda: W.make_repbn8_state_dict(SEED)}
    gens.update({n: (lambda n=n: W.make_variant_state_dict(n, SEED)) for n in W.VARIANT_NAMES})
    gens["cvit_GGCA_ADD_DConv"] = lambda: W.make_dconv_state_dict(SEED)
    gens.update({n: (lambda n=n: W.make_other_state_dict(n, SEED)) for n in W.OTHER_NAMES})
    return gens


def rows(sd) -> list:
    sums = W.state_dict_checksums(sd)
    return [[k, list(v.shape), *sums[k]] + ([str(v.dtype)] if str(v.dtype) != "float32" else []) for k, v in sd.items()]


def pack(by_name: dict) -> dict:
    """{name: rows} -> the fixture: distinct rows once, in order of first use."""
    index, classes = {}, {}
    for name, rs in by_name.items():
        classes[name] = [index.setdefault(json.dumps(r), len(index)) for r in rs]
    return {"tensors": [json.loads(r) for r in index], "classes": classes}


def expand(fixture: dict) -> dict:
    """The fixture -> {name: rows}."""
    return {name: [fixture["tensors"][i] for i in idx] for name, idx in fixture["classes"].items()}


def dumps(fixture: dict) -> str:
    """Compact JSON, eight tensors or one class per line."""
    js = lambda o: json.dumps(o, separators=(",", ":"))  # noqa: E731
    t = fixture["tensors"]
    lines = [",".join(js(r) for r in t[i:i + 8]) for i in range(0, len(t), 8)]
    classes = [f"{js(n)}:{js(idx)}" for n, idx in fixture["classes"].items()]
    return '{"tensors":[\n' + ",\n".join(lines) + '\n],"classes":{\n' + ",\n".join(classes) + "\n}}\n"


def main():
    fixture = pack({name: rows(make()) for name, make in generators().items()})
    OUT.write_text(dumps(fixture))
    print(f"wrote {OUT.relative_to(REPO)}: {len(fixture['classes'])} classes, {len(fixture['tensors'])} distinct tensors, "
          f"{OUT.stat().st_size} bytes")


if __name__ == "__main__":
    main()
