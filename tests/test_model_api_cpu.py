"""The public surface of `Model` is frozen: every public attribute's signature and docstring against
tests/golden/model_api.json.  `python tests/test_model_api_cpu.py` rewrites that file from the tree it runs in."""
import hashlib
import inspect
import json
import os

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "model_api.json")


def _surface() -> dict:
    from randlanet.model import Model
    out = {}
    for name in sorted(vars(Model)):
        if name.startswith("_"):
            continue
        attr = inspect.getattr_static(Model, name)
        fn = attr.fget if isinstance(attr, property) else getattr(Model, name)
        out[name] = {"signature": str(inspect.signature(fn)),
                     "doc_sha256": hashlib.sha256((fn.__doc__ or "").encode()).hexdigest()}
    return out


def test_public_surface_is_unchanged():
    with open(GOLDEN) as f:
        golden = json.load(f)
    surface = _surface()
    assert sorted(surface) == sorted(golden)
    for name, entry in golden.items():
        assert surface[name] == entry, name


if __name__ == "__main__":
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(GOLDEN), "..", "..", "3d_recognizer_amd"))
    with open(GOLDEN, "w") as f:
        json.dump(_surface(), f, indent=1, sort_keys=True)
        f.write("\n")
