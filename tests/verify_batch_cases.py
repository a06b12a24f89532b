"""Fixtures and restatements shared by the batch verifier's tests (test_verify_batch_cpu.py, test_gpu_verify_batch.py); a plain
helper module like msm_cases.py.

The three golden EVM proofs under the reference's key, the multipliers of csrc/verify_batch_plan.h restated over
merkle_sum_tree.keccak256_python, the bound on the pairing checks of a rejected batch, and the tampers of the GPU test."""
import json
import os

from conftest import GOLDEN

H = lambda s: int(s, 16)
GOLDEN_PROOFS = ("k6_inclusion_proof_solidity_calldata.json", "gpu_proof_entry16_user0.json", "gpu_proof_entry16_user0_cpp.json")


def reference_key():
    """(params, vk): the reference's SRS and the verifying key of its verifier contract, as test_gpu_api.py builds it"""
    from circuits_halo2_amd import api, params as PM
    tr = json.load(open(os.path.join(GOLDEN, "k6_verifier_trace.json")))["vk"]
    comm = [(H(a), H(b)) for a, b in tr["commitments"]]
    vk = api.VerifyingKey(11, 2, comm[:11], comm[11:], H(tr["vk_digest"]))
    return PM.ParamsKZG.read(open(os.path.join(GOLDEN, "hermez-raw-11"), "rb")), vk


def golden_proofs():
    """[(proof bytes, [public inputs as integers])] of the three fixtures"""
    out = []
    for name in GOLDEN_PROOFS:
        cd = json.load(open(os.path.join(GOLDEN, name)))
        out.append((bytes.fromhex(cd["proof"][2:]), [H(x) for x in cd["public_inputs"]]))
    return out


def cycled(n):
    """the golden proofs cycled to n: (proofs, instance columns)"""
    g = golden_proofs()
    return [g[i % len(g)][0] for i in range(n)], [list(g[i % len(g)][1]) for i in range(n)]


def instance_words(instances) -> bytes:
    """an instance column as sv_verify_batch takes it: 32-byte Montgomery words"""
    from circuits_halo2_amd import verifier as V
    return b"".join(V._fr_bytes(int(v)) for v in instances)


def multipliers(vk_digest: int, proofs, instances_list, entropy=None):
    """(seed, [r_i]) of csrc/verify_batch_plan.h, restated:
    seed = Keccak256(vk_digest || N || for each proof: len || proof || n_instances || instances || entropy or 32 zero bytes),
    r_i = the low 128 bits of Keccak256(seed || i) read as a little-endian integer, 0 replaced by 1"""
    from circuits_halo2_amd.merkle_sum_tree import keccak256_python
    buf = int(vk_digest).to_bytes(32, "big") + len(proofs).to_bytes(4, "little")
    for proof, inst in zip(proofs, instances_list):
        buf += len(proof).to_bytes(8, "little") + bytes(proof) + len(inst).to_bytes(4, "little") + instance_words(inst)
    buf += bytes(entropy) if entropy is not None else bytes(32)
    seed = keccak256_python(buf)
    rs = [int.from_bytes(keccak256_python(seed + i.to_bytes(4, "little"))[:16], "little") or 1 for i in range(len(proofs))]
    return seed, rs


def pairing_bound(n: int, bad: int) -> int:
    """1 for a batch without a bad proof, else 1 + 2 |bad| ceil(log2 n)"""
    return 1 if bad == 0 else 1 + 2 * bad * (n - 1).bit_length()


# ------------------------------------------------------------------ tampers (EVM proofs: 2144 bytes; the evaluations start at 0x380)
R = 21888242871839275222246405745257275088548364400416034343698204186575808495617


def _flip_evaluation(proof, inst):
    p = bytearray(proof)
    p[0x380 + 32 * 5 + 31] ^= 0x04
    return bytes(p), inst


def _off_curve(proof, inst):
    p = bytearray(proof)
    p[32:64] = (int.from_bytes(proof[32:64], "big") ^ 1).to_bytes(32, "big")     # y of the first commitment
    return bytes(p), inst


def _public_input(proof, inst):
    return proof, [inst[0], inst[1], (inst[2] + 1) % R, inst[3]]


def _short(proof, inst):
    return proof[:-1], inst


def _scalar_r(proof, inst):
    p = bytearray(proof)
    p[0x380:0x3a0] = R.to_bytes(32, "big")
    return bytes(p), inst


TAMPERS = {"evaluation": _flip_evaluation, "off_curve": _off_curve, "public_input": _public_input, "short": _short, "scalar_r": _scalar_r}
