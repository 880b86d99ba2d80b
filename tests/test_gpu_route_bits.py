"""Three IRLS iterations on every route through the host code of the banded direct solver return the recorded BITS.

The host side of bcr.hip decides which launches a solve is made of (irotavg_amd/csrc/bcr_route.hpp). A change there must
not move a single bit: per case of tests/golden/make_route_bits.py -- small shapes of band_cases / closure_cases with their
environment switches, blocks of 8 / 12 / 16 / 24 / 32: the plain route with the unit-weight store filled and then served,
a mixed level 1, IROTAVG_BCR_NO_FUSED_ASM, IROTAVG_BCR_UP_CAP=0, IROTAVG_BCR_NO_TOP16, IROTAVG_BCR_NO_UNIT_FACTOR, two
levels under a single-workgroup top, levels launched one by one, a one-level handle, closures -- the iteration count, the
score trace, SHA-256 of the rotations and of the weights, direct_info() and the counters of stats() are compared with
tests/golden/route_bits.json for equality. There is no tolerance.

The JSON was recorded on an MI355X by make_route_bits.py at the commit before the route decision got a place of its own;
every case was recorded twice and all were deterministic. (A mixed level 1 needs the 256 compute units the cases are sized
for: on another device direct_info differs and the case fails with both shapes in the message.)
"""
import json
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_route_bits as RB  # noqa: E402

pytestmark = pytest.mark.gpu

with open(os.path.join(HERE, "golden", "route_bits.json")) as fh:
    GOLDEN = json.load(fh)
MUST = ("plain-b8", "plain-b16", "plain-b24", "mixed-b8", "no-fused-asm-b8", "up-cap-0-b8", "no-top16-b8")


def test_the_recording_covers_every_case():
    assert sorted(GOLDEN) == sorted(s[0] for s in RB.SPECS)
    for name in MUST:
        assert isinstance(GOLDEN[name], list), name           # (these may not be left out as non-deterministic)
    # the store was filled by the first call and served the second one where the route keeps one
    for name in ("plain-b8", "plain-b16", "plain-b24", "mixed-b8"):
        first, second = GOLDEN[name]
        assert first["info"]["unit_factor"] == 1 and first["info"]["unit_factor_solves"] == 0
        assert second["info"]["unit_factor_solves"] == 1


@pytest.mark.parametrize("spec", [s for s in RB.SPECS if isinstance(GOLDEN.get(s[0]), list)], ids=lambda s: s[0])
def test_three_iterations_return_the_recorded_bits(spec):
    got = json.loads(json.dumps(RB.record(spec)))              # (as the file holds it)
    want = GOLDEN[spec[0]]
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        for key in ("info", "stats", "iters", "scores", "Q", "w"):
            assert g[key] == w[key], (spec[0], "call %d" % k, key, g[key], w[key])
