#!/usr/bin/env python3
"""SHA-256 digests of what the five step-term suites compare the kernels against (tests/step_terms.py and the term modules
ball_contact_ref, leg_contact_ref, ground_contact_ref, joint_drive_ref, body_wrench_ref): CPU only, the oracle's two builds and numpy.
Two trees that print the same lines hold the kernels to the same references, kept envs and bars:

  python tools/step_term_digests.py > digests.txt        (profiles/step_term_harness_digests.txt)

One line per case: sha256[:16] over every array of ref.out64 and of ref.out32 (keys sorted), ref.kept and the repr of the sorted
case_bars(ref) items; the wrench cases add unl64, unl32, words64 and the repr of the sorted response_bars(ref) items.  One line per
planted slip: the outputs planted() returns, and its decision words where it returns some.  The shared names are looked up in
tests/step_terms.py, and in tests/ball_contact_ref.py on a tree from before that module."""
import hashlib
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np   # noqa: E402

from bez_isaacgym_amd import abi   # noqa: E402
from tests import ball_contact_ref as B   # noqa: E402
from tests import body_wrench_ref as W   # noqa: E402
from tests import ground_contact_ref as G   # noqa: E402
from tests import joint_drive_ref as J   # noqa: E402
from tests import leg_contact_ref as L   # noqa: E402

try:
    from tests import step_terms as S   # noqa: E402
except ImportError:
    S = B

N = 1000
NS = abi.FLAG_NO_SELF_COLLISION
# the oracle cases of tests/test_gpu_ball_contact.py, which has no CASES list: name -> reference(*args)
BALL_CASES = {}
for _a in S.ASSETS:
    for _dr in (False, True):
        BALL_CASES["free-%s %s" % ("dr" if _dr else "plain", _a)] = ("free", _a, N, 2, _dr, 0)
for _a in S.ASSETS:
    for _dr in (False, True):
        BALL_CASES["free1-%s %s" % ("dr" if _dr else "plain", _a)] = ("free", _a, N, 1, _dr, NS)
for _a in S.ASSETS:
    BALL_CASES["kick %s" % _a] = ("kick", _a, N, 2, False, 0)
for _s in (1, 3, 4):
    BALL_CASES["free-s%d default" % _s] = ("free", "default", N, _s, False, 0)
BALL_CASES["dense200 default"] = ("free", "default", 200, 2, False, 0)
BALL_CASES["sparse default"] = ("sparse", "default", 200, 2, False, 0)


def _arrays(h, d):
    for k in sorted(d):
        h.update(np.ascontiguousarray(d[k]).tobytes())


def case_digest(ref, wrench=False):
    h = hashlib.sha256()
    _arrays(h, ref.out64); _arrays(h, ref.out32)
    h.update(np.ascontiguousarray(ref.kept).tobytes())
    h.update(repr(sorted(S.case_bars(ref).items())).encode())
    if wrench:
        _arrays(h, ref.unl64); _arrays(h, ref.unl32)
        h.update(np.ascontiguousarray(ref.words64).tobytes())
        h.update(repr(sorted(W.response_bars(ref).items())).encode())
    return h.hexdigest()[:16]


def slip_digest(planted):
    h = hashlib.sha256()
    _arrays(h, planted[1])
    for words in planted[2:]:
        h.update(np.ascontiguousarray(words).tobytes())
    return h.hexdigest()[:16]


def main():
    def line(suite, name, digest):
        print("%-7s %-40s %s" % (suite, name, digest), flush=True)
    for name, args in BALL_CASES.items():
        line("ball", name, case_digest(B.reference(*args)))
    for suite, M in (("leg", L), ("ground", G), ("joint", J)):
        for case in M.CASES:
            line(suite, M.case_name(*case), case_digest(M.reference(*case)))
    for name, kw in W.CASES.items():
        line("wrench", name, case_digest(W.reference(**kw), wrench=True))
    for suite, M in (("leg", L), ("ground", G), ("joint", J), ("wrench", W)):
        for slip in M.SLIPS:
            line(suite, "slip " + slip, slip_digest(M.planted(slip)))


if __name__ == "__main__":
    main()
