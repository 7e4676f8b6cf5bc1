"""Generates tests/golden/reference_public_surface.json — the reference's public surface as tests/test_boundary_mirror.py
compares it with the mirror csrc/host/nos_reference_api.hpp.

    python tests/golden/make_boundary_golden.py <reference checkout>/nonlinear_optimizer

Reads the reference's headers (options.h, loss_function.h, the solvers' types.h and base-class headers) where they lie
and stores one SHA-256 fingerprint per fact that public_surface() extracts from them.  No header text is stored.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests.test_boundary_mirror import GOLDEN, fingerprints, reference_surface  # noqa: E402

if len(sys.argv) != 2 or not os.path.isdir(sys.argv[1]):
    raise SystemExit(__doc__)
fixture = {
    "source": "ChanghyeonKim93/nonlinear_optimizer_for_slam @ 2025-09-12, nonlinear_optimizer/ headers",
    "sha256": fingerprints(reference_surface(sys.argv[1])),
}
with open(GOLDEN, "w") as f:
    json.dump(fixture, f, indent=1)
    f.write("\n")
print("wrote %s (%d facts)" % (os.path.relpath(GOLDEN), len(fixture["sha256"])))
