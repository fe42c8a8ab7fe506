"""Writes tests/golden/ir_preprocess.npz: three small uint8-derived images and what the REFERENCE's own
src/models/cnnBasedThermalInfraredDA.py returns for each of its nine pre-processing methods on them (its file is executed as it is, with
the stand-in modules of tests/_ir_preprocess_oracle.py for the packages it imports and this toolchain lacks).

    python tests/golden/make_ir_preprocess_golden.py [<path to a checkout of the reference>]      (default: $HALLUCIDET_REFERENCE)

Only data the reference produced is stored; none of its text."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import _ir_preprocess_oracle as O  # noqa: E402


def inputs():
    skewed = torch.stack([O.plane_u8("skewed", 37, 53, seed=11 + c) for c in range(3)]).float() / 255.0
    narrow = O.plane_u8("narrow", 48, 64, seed=21)[None].float() / 255.0
    const = O.plane_u8("const", 16, 16)[None].float() / 255.0
    return {"skewed": skewed, "narrow": narrow, "const": const}


def main(root):
    cls = O.load_reference(root)
    if cls is None:
        raise SystemExit("no src/models/cnnBasedThermalInfraredDA.py under %s" % root)
    out = {}
    for name, x in inputs().items():
        out["in_" + name] = x.numpy()
        for m in O.METHODS:
            out["%s_%s" % (m, name)] = O.run_reference(cls, m, x).numpy()
    path = os.path.join(HERE, "ir_preprocess.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.environ.get("HALLUCIDET_REFERENCE", "/root/reference"))
