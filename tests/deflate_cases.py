"""Inputs of the device gzip tests (tests/test_deflate_host_model.py on the CPU, tests/test_gpu_deflate.py on the GPU): the
smallest texts at which a chunked one-candidate LZ77 + Huffman coder can go wrong.  `cases(C)` yields
(name, data, flag sets); C is pf_gzip_device_chunk_bytes()."""
import functools
import gzip
import random

FIXED_ONLY, DYNAMIC_ONLY, LITERALS_ONLY = 1, 2, 4
ALL = (0, FIXED_ONLY, DYNAMIC_ONLY)

LENGTH_EDGES = (3, 4, 10, 11, 12, 18, 19, 34, 35, 66, 67, 130, 131, 257, 258)
DISTANCE_EDGES = (1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073,
                  4097, 6145)
FAR_DISTANCE_EDGES = (8193, 12289, 16385, 24577, 32768)
RUN_LENGTHS = (1, 2, 3, 4, 5, 257, 258, 259, 260, 261, 516, 517)


def _rand(seed, n):
    return random.Random(seed).randbytes(n)


def length_edge(L):
    """300 random bytes R, a byte absent from R, R[:L], then a byte different from R[L]: a match of exactly L"""
    while True:
        R = _rand(1000 + L, 300)
        absent = [b for b in range(256) if b not in R]
        if absent:
            break
    return R + bytes([absent[0]]) + R[:L] + bytes([(R[L] + 1) & 0xFF])


def distance_edge(D):
    """an 8-byte block, random filler, the block again exactly D bytes after its first occurrence"""
    rng = random.Random(2000 + D)
    block = rng.randbytes(8)
    if D >= 8:
        return block + rng.randbytes(D - 8) + block
    return (block[:D] * 4)[:D + 8]          # the second occurrence overlaps the first: period D


def fibonacci_counts(C):
    """byte value i occurs F(i) times, i = 1..m, m the largest with F(m + 2) - 1 <= C: an unlimited Huffman code of
    these frequencies is m - 1 >= 16 bits deep"""
    F = [0, 1, 1]
    while len(F) < 64:
        F.append(F[-1] + F[-2])
    m = max(i for i in range(1, 40) if F[i + 2] - 1 <= C)
    assert m >= 17
    data = bytearray()
    for i in range(1, m + 1):
        data += bytes([i]) * F[i]
    random.Random(7).shuffle(data)
    return bytes(data)


@functools.lru_cache(maxsize=None)
def real_shapes(C):
    """about 5 C bytes of each of the three files' text: kmers_to_hashes rows, hashes_to_patterns rows at 100 strains
    with NaN cells, kmers.tsv rows -- from a small synthetic pangenome through the CPU oracle"""
    from oracle import oracle as po
    from panfeed_amd import synth
    clusters = synth.generate(10, 100, first=4200, flank=10, mean_len=300, min_len=80, max_len=600, n_rate=0.02,
                              paralog_rate=0.05)
    names = clusters[0].names
    run = po.OracleRun(klength=21, stroi={names[1], names[5], names[50]}, canon=True, consider_missing=True,
                       patfilt=True, maf=0.01)
    run.feed([c.record() for c in clusters])
    kmers_tsv, kmers_to_hashes, hashes_to_patterns = (t.encode() for t in run.texts())
    assert b"\t\t" in hashes_to_patterns
    want = 5 * C
    return {name: (text * (want // len(text) + 1))[:want + 13]
            for name, text in (("kmers_to_hashes", kmers_to_hashes), ("hashes_to_patterns", hashes_to_patterns),
                               ("kmers_tsv", kmers_tsv))}


def cases(C):
    for n in (0, 1, 2, 3, 4):                                                   # 1
        yield f"short{n}", b"pqrs"[:n], ALL
    every = bytes(range(256))
    yield "all_bytes_twice", every + every, ALL                                 # 2
    for n in RUN_LENGTHS + (C - 1, C, C + 1, 2 * C + 3):                          # 3
        yield f"run{n}", b"a" * n, ALL
        yield f"period2_{n}", (b"0\t" * (n // 2 + 1))[:n], ALL
    for L in LENGTH_EDGES:                                                      # 4
        yield f"len{L}", length_edge(L), ALL
    for D in DISTANCE_EDGES + tuple(d for d in FAR_DISTANCE_EDGES if d < C - 16):   # 5
        yield f"dist{D}", distance_edge(D), ALL
    yield "incompressible", _rand(3, 3 * C + 17), (0,)                          # 6
    fib = fibonacci_counts(C)                                                   # 7
    yield "fibonacci", fib, (LITERALS_ONLY | DYNAMIC_ONLY, DYNAMIC_ONLY)
    perm = bytearray(every)
    random.Random(8).shuffle(perm)
    yield "no_distance_symbol", bytes(perm), (DYNAMIC_ONLY,)                    # 8
    yield "one_literal_symbol", b"a" * 64, (LITERALS_ONLY | DYNAMIC_ONLY,)      # 9
    for name, text in real_shapes(C).items():                                   # 10
        yield f"shape_{name}", text, ALL


def flat_cases(C):
    return [(f"{name}-f{flags}", data, flags) for name, data, flagset in cases(C) for flags in flagset]


def check_members(data, members, C):
    """any gzip reader gets back the text: gzip.decompress walks all members and checks every CRC32 and ISIZE"""
    if not data:
        assert len(members) == 0
        return
    assert gzip.decompress(bytes(members)) == data


def incompressible_cap(n, C):
    return n + 32 * -(-n // C) + 32
