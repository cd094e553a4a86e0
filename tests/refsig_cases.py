"""Seeded inputs of the reference-from-bases tests (tests/test_refsig_host.py, tests/test_refsig_gpu.py) and of their fixture
(tests/golden/seq_to_sig_ref.npz, scripts/make_golden_refsig.py): the cases every form of ri_seq_to_sig (src/rsig.cpp:7-41) is held to.
A case is (name, sequences as bytes, model float32 of 4^k levels, k): one call of rawdtw_reference_from_bases.  The fixture records the
SHA-256 of all of them, so a generator that drifts fails loudly instead of comparing against answers to other questions."""
import functools
import hashlib

import numpy as np

S_LENS = (1, 2, 63, 64, 65, 4095, 4096, 4097, 70_001)  # around a step of 64, around 64 steps, and many steps
ADVERSARIAL = np.array([1.0, 1.5, 2.0 ** -30, 2.0 ** 20, 0.0, 3 * 2.0 ** -25, 2.0 ** -52, 0.75], np.float32)
NEGATIVE = np.array([-1.0, 0.0, -0.5, -3.25, 0.0, -2.0 ** -20, -7.0, -0.125], np.float32)
LONG = "long300000_k6"
NEG = "negative_model_k3"


def _bases(rng, n) -> bytes:
    return np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, n)].tobytes()


@functools.lru_cache(maxsize=1)
def cases():
    from rawalign_amd.synth import make_pore_model

    rng = np.random.default_rng(20261019)
    out = []
    for k in (3, 6, 9):
        pore = make_pore_model(k, seed=100 + k)
        # s_len 0 twice (no base at all, k - 1 bases), then every length of S_LENS
        seqs = [b"", _bases(rng, k - 1)] + [_bases(rng, n + k - 1) for n in S_LENS]
        out.append((f"lengths_k{k}", seqs, pore, k))
        # N, other letters and lower case, also inside the first and the last k bases
        s = bytearray(_bases(rng, 700))
        for at in (0, 1, k - 1, k, 350, 351, 352, 700 - k - 1, 700 - k, 699):
            s[at] = ord("N")
        for at in rng.integers(0, 700, 60):
            s[at] = ord(bytes([s[at]]).lower())
        s[2], s[400], s[698] = ord("n"), ord("R"), ord("-")
        allN = b"N" * 100
        out.append((f"ambiguous_k{k}", [bytes(s), bytes(s).lower(), allN, b"acgtNNNNNNNNNNNNacgtACGTTTGA" * 9], pore, k))
    pore6 = make_pore_model(6, seed=106)
    out.append(("one_letter_k6", [b"A" * 500, b"t" * 70, b"G" * 6], pore6, 6))  # std_dev 0: NaN throughout
    lens = [int(x) for x in rng.integers(0, 900, 37)]
    lens[0], lens[5], lens[17], lens[36] = 0, 3, 0, 5  # empty ones and ones below k
    out.append(("mixed37_k6", [_bases(rng, n) for n in lens], pore6, 6))

    def model3(levels, seed):
        r = np.random.default_rng(seed)
        return levels[r.integers(0, len(levels), 64)].astype(np.float32)
    out.append(("adversarial_model_k3", [_bases(rng, 3000)], model3(ADVERSARIAL, 7), 3))
    out.append((NEG, [_bases(rng, 3000)], model3(NEGATIVE, 8), 3))
    out.append((LONG, [_bases(rng, 300_000)], make_pore_model(6), 6))
    return out


NT4 = np.full(256, 4, np.uint8)
for _i, _c in enumerate(b"ACGT"):
    NT4[_c] = NT4[ord(chr(_c).lower())] = _i


def levels(seq: bytes, pore, k: int, strand: int) -> np.ndarray:
    """the model's level of every output element, in emission order (rsig.cpp:14-29)"""
    c = NT4[np.frombuffer(seq, np.uint8)].astype(np.int64)
    if strand:
        c = c[::-1]
    c = np.where(c < 4, (3 ^ c) if strand else c, 0)  # an ambiguous base shifts 00 in
    n = len(c) - k + 1
    if n <= 0:
        return np.zeros(0, np.float32)
    idx = np.zeros(n, np.int64)
    for j in range(k):
        idx = idx << 2 | c[j:j + n]
    return np.ascontiguousarray(pore, np.float32)[idx]


def canonical(x) -> np.ndarray:
    """the floats' bits with every NaN as one value: a NaN's sign and payload are not part of the contract"""
    x = np.ascontiguousarray(x, np.float32)
    b = x.view(np.uint32).copy()
    b[np.isnan(x)] = 0x7FC00000
    return b


def same(a, b) -> bool:
    return len(a) == len(b) and np.array_equal(canonical(a), canonical(b))


def inputs_sha256(cs) -> str:
    h = hashlib.sha256()
    for name, seqs, pore, k in cs:
        h.update(name.encode() + bytes([k]))
        for s in seqs:
            h.update(len(s).to_bytes(8, "little") + s)
        h.update(np.ascontiguousarray(pore, np.float32).tobytes())
    return h.hexdigest()


def outputs_sha256(arrays) -> bytes:
    """of one case in one form: every sequence's strand 1 then strand 0, lengths included"""
    h = hashlib.sha256()
    for a in arrays:
        h.update(len(a).to_bytes(8, "little") + canonical(a).tobytes())
    return h.digest()
