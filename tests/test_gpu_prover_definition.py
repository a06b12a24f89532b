"""The prover drivers against the definition (tests/prover_definition.py), k = 9.  The verifier accepts any proof whose committed
polynomials satisfy the constraints on the usable rows and is blind to the blinding rows; under a known ChaCha20 key and a known
tau the first nine commitments of a proof are pinned here bit for bit, blinding rows included.  Under fresh keys the proofs of a
group must differ at EVERY point position (a shared key or a missing draw shows as an equal point), and no advice or permuted
lookup column may be committed unblinded.  No tolerance: every comparison is equality of points.  (The compiled driver under a
fixed key: test_gpu_prover.py::test_cpp_prover_under_a_fixed_blinding_key_equals_the_python_driver.)"""
import itertools
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import prover_definition as D
from test_gpu_prover import make_setup, seeded_rng

pytestmark = pytest.mark.gpu

KEY = seeded_rng(101)


@pytest.fixture(scope="module")
def setup():
    s = make_setup(9)
    s["advice"] = [s["dev"](c) for c in s["asg"]["advice"]]
    yield s
    s["params"].free()


@pytest.fixture(scope="module")
def evm_points(setup):
    """the Python driver's EVM-transcript proof under KEY, checked against the definition: its 16 points"""
    s = setup
    proof = s["prover"].create_proof(s["params"], s["pk"], s["advice"], s["asg"]["instances"], KEY)
    return D.check_proof(proof, s["asg"], s["k"], s["tau"], KEY, s["vk"])


@pytest.fixture(scope="module")
def unblinded_points(setup):
    """what a0 a1 a2 a' s' commit to with their blinding rows left zero (host)"""
    s = setup
    cols = D.witness_columns(s["asg"], s["k"])
    return {name: D.commit_at_tau(col, s["tau"], s["k"]) for name, col in cols.items()}


def test_python_driver_evm_transcript(setup, evm_points):
    s = setup
    key2 = seeded_rng(102)
    proof = s["prover"].create_proof(s["params"], s["pk"], s["advice"], s["asg"]["instances"], key2)
    other = D.check_proof(proof, s["asg"], s["k"], s["tau"], key2, s["vk"])
    assert all(other[name] != evm_points[name] for name in other)          # another key: another point at every position


def test_python_driver_blake2b_transcript(setup, evm_points):
    """other challenges, so other grand products; the columns that wait for no challenge commit to the EVM run's points"""
    s = setup
    P = s["prover"]
    proof = P.create_proof(s["params"], s["pk"], s["advice"], s["asg"]["instances"], KEY, transcript=P.Blake2bWrite())
    got = D.check_proof(proof, s["asg"], s["k"], s["tau"], KEY, s["vk"], flavour="blake2b")
    for name in ("a0", "a1", "a2", "pin", "ptab", "random"):
        assert got[name] == evm_points[name], name
    for name in ("z0", "z1", "lz"):
        assert got[name] != evm_points[name], name


def test_python_driver_with_the_quotient_on_the_extended_domain(setup, evm_points):
    s = setup
    P, dev = s["prover"], s["dev"]
    pk_ext = P.ProvingKey(s["params"], s["k"], [dev(c) for c in s["asg"]["fixed"]], [dev(c) for c in s["asg"]["sigma"]],
                          quotient_domain="extended")
    proof = P.create_proof(s["params"], pk_ext, s["advice"], s["asg"]["instances"], KEY)
    assert D.check_proof(proof, s["asg"], s["k"], s["tau"], KEY, s["vk"]) == evm_points


def _python_twice(s):
    return [("evm", s["prover"].create_proof(s["params"], s["pk"], s["advice"], s["asg"]["instances"], None)) for _ in range(2)]


def _native_twice(s, flavour="evm"):
    return [(flavour, s["prover"].create_proof_native(s["params"], s["pk"], s["advice"], s["asg"]["instances"], flavour)) for _ in range(2)]


def _native_from_four_threads(s, combine):
    """the pattern of test_gpu_prover.py::test_native_proofs_from_several_threads: each thread on its own stream, one proof each,
    all on the same advice and instances"""
    import threading
    import torch
    P = s["prover"]
    P.create_proof_native(s["params"], s["pk"], s["advice"], s["asg"]["instances"])          # the native key, made once
    torch.cuda.synchronize()
    proofs, errors = [], []
    gate = threading.Barrier(4)

    def worker():
        try:
            with torch.cuda.stream(torch.cuda.Stream()):
                gate.wait()
                proofs.append(("evm", P.create_proof_native(s["params"], s["pk"], s["advice"], s["asg"]["instances"], combine=combine)))
        except Exception as e:  # noqa: BLE001
            gate.abort()
            errors.append(repr(e))
    threads = [threading.Thread(target=worker) for _ in range(4)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    assert len(proofs) == 4
    return proofs


GROUPS = {
    "python driver twice": _python_twice,
    "native driver twice on one thread": _native_twice,
    "native driver twice, Blake2b transcript": lambda s: _native_twice(s, "blake2b"),
    "native driver from four threads, combined commitments": lambda s: _native_from_four_threads(s, True),
    "native driver from four threads": lambda s: _native_from_four_threads(s, False),
}


@pytest.mark.parametrize("group", list(GROUPS))
def test_fresh_keys_give_fresh_points_everywhere(setup, unblinded_points, group):
    """proofs under keys from the OS: each verifies; at each of the 16 point positions (14 commitments, W, W') the proofs of the
    group are pairwise different; none of a0 a1 a2 a' s' is the commitment of the column with its blinding rows zero"""
    from oracle import summa_verifier as SV
    s = setup
    proofs = GROUPS[group](s)
    points = []
    for flavour, proof in proofs:
        assert SV.verify(proof, s["asg"]["instances"], s["vk"], flavour=flavour)
        pts = D.proof_points(proof, flavour)
        assert len(pts) == 16
        points.append(pts)
    for a, b in itertools.combinations(range(len(points)), 2):
        for (name, p), (_, q) in zip(points[a], points[b]):
            assert p != q, f"{group}: proofs {a} and {b} carry the same point at {name}"
    for i, pts in enumerate(points):
        for name, p in pts:
            if name in unblinded_points:
                assert p != unblinded_points[name], f"{group}: proof {i} commits to {name} unblinded"
