"""The two host-checkable helpers a search wave's head relies on (reart_amd/csrc/internal.h), compiled for the HOST and run here:

  * reart_div_by_magic(n, d, reart_div_magic(d)) against n / d: the wave splits its (batch, query group) pair with one
    multiply-high and one correction, so it must be exact for every query-group count and every pair.  Walked: EVERY pair
    0 .. SEARCH_ITEM_PAIR_MASK for every nqg <= 64; for every larger nqg up to SEARCH_ITEM_PAIR_MASK + 1 (a launch has at least
    one pair per group, so no larger count fits an item word) the boundaries k * nqg - 1, k * nqg, k * nqg + 1 of every k; and --
    launches without item words take the pair from an order array, any int -- the same boundaries at the top of the 31-bit
    range plus 20 M pseudo-random (n, d) over all 32 bits.
  * reart_search_off32 (picks the kernel whose frame offsets are 32-bit products) against a direct computation of the largest
    byte offset a wave forms, for shapes on both sides of 2^31 bytes per array.
"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "reart_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

SRC = r"""
#include "internal.h"
#include <cstdio>
#include <cstdlib>
#include <cstdint>
static unsigned long long bad = 0, seen = 0;
static inline void one(unsigned n, unsigned d, unsigned m) {
    const unsigned q = reart_div_by_magic(n, d, m);
    ++seen;
    if (q != n / d || n - q * d != n % d) { if (bad++ < 10) std::printf("MISMATCH n=%u d=%u m=%u got %u want %u\n", n, d, m, q, n / d); }
}
static void edges(unsigned d, unsigned long long top) {
    const unsigned m = reart_div_magic(d);
    for (unsigned long long e = 0; e <= top + 1; e += d)
        for (long long o = -1; o <= 1; ++o) {
            const long long n = (long long)e + o;
            if (n >= 0 && (unsigned long long)n <= top) one((unsigned)n, d, m);
        }
    one((unsigned)top, d, m);
}
int main(int argc, char **argv) {
    if (argc > 1 && argv[1][0] == 'o') {                 // off32 B P1 Ppad K ...
        for (int k = 2; k + 3 < argc; k += 4)
            std::printf("%d\n", reart_search_off32(atoll(argv[k]), atoll(argv[k + 1]), atoll(argv[k + 2]), atoi(argv[k + 3])) ? 1 : 0);
        return 0;
    }
    const unsigned mask = SEARCH_ITEM_PAIR_MASK;
    for (unsigned d = 1; d <= 64; ++d) {
        const unsigned m = reart_div_magic(d);
        for (unsigned n = 0; n <= mask; ++n) one(n, d, m);
    }
    for (unsigned d = 65; d <= mask + 1u; ++d) edges(d, mask);
    // order arrays (no item words): pairs up to INT_MAX; the top of that range, every k would take too long
    for (unsigned d = 1; d <= 4096; ++d) {
        const unsigned m = reart_div_magic(d);
        const unsigned top = 0x7fffffffu, k0 = top / d;
        for (unsigned k = k0 > 4 ? k0 - 4 : 0; k <= k0; ++k)
            for (int o = -1; o <= 1; ++o) {
                const long long n = (long long)k * d + o;
                if (n >= 0 && n <= (long long)top) one((unsigned)n, d, m);
            }
        one(top, d, m);
    }
    uint64_t s = 0x9E3779B97F4A7C15ull;
    for (int k = 0; k < 20000000; ++k) {
        s ^= s << 13; s ^= s >> 7; s ^= s << 17;
        unsigned n = (unsigned)s, d = (unsigned)(s >> 32);
        if ((k & 3) == 1) d >>= 16;
        if ((k & 3) == 2) d >>= 24;
        if (d == 0) d = 1;
        one(n, d, reart_div_magic(d));
    }
    for (unsigned d : {1u, 2u, 3u, 0x7fffffffu, 0x80000000u, 0x80000001u, 0xfffffffeu, 0xffffffffu})
        for (unsigned n : {0u, 1u, 0x7ffffffeu, 0x7fffffffu, 0x80000000u, 0xfffffffeu, 0xffffffffu}) one(n, d, reart_div_magic(d));
    std::printf("checked %llu mismatches %llu mask %u\n", seen, bad, mask);
    return bad ? 1 : 0;
}
"""


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    if not (os.path.exists(HIPCC) or shutil.which(HIPCC)):
        pytest.fail(f"{HIPCC} not found: the helpers are compiled from internal.h")
    d = tmp_path_factory.mktemp("item_div")
    src, exe = d / "item_div.hip", d / "item_div"
    src.write_text(SRC)
    # host side only: the same header the kernels include, REART_HD functions as host code
    subprocess.check_call([HIPCC, "--cuda-host-only", "-O2", "-std=c++17", f"-I{CSRC}", str(src), "-o", str(exe)],
                          stderr=subprocess.DEVNULL)
    return str(exe)


def test_reciprocal_division_is_exact_for_every_group_count_and_pair(prog):
    r = subprocess.run([prog], capture_output=True, text=True, timeout=300)
    print(r.stdout[-2000:])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    last = r.stdout.strip().splitlines()[-1].split()
    assert last[0] == "checked" and int(last[1]) > 64 * (1 << 21) and int(last[3]) == 0
    assert int(last[5]) == (1 << 21) - 1


def _largest_byte_offset(B, P1, Ppad, K, box=16):
    """The last byte a search wave can address in each per-frame array, from the index expressions themselves."""
    q = (((B - 1) * P1 + (P1 - 1)) * 3 + 2) * 4                        # queries [B][P1][3]
    rec = (((B - 1) * P1 + (P1 - 1)) * K + (K - 1)) * 4                # seeds / records [B][P1][K]
    tgt = (((B - 1) * 3 + 2) * Ppad + (Ppad - 1)) * 4                  # targets [B][3][Ppad]
    bx = (((B - 1) * (Ppad // box) + (Ppad // box - 1)) * 8 + 7) * 4   # boxes [B][Ppad / 16][8]
    return max(q, rec, tgt, bx)


SHAPES = [
    (19, 4096, 4096, 1), (19, 4096, 4096, 3), (3, 330, 336, 3), (1, 1, 16, 1),
    # around 2^31 bytes of queries / targets: B * P1 * 12 = 2^31 at B * P1 = 178 956 970.67
    (1, 178956970, 16, 1), (1, 178956971, 16, 1), (2, 89478485, 16, 1), (2, 89478486, 16, 1),
    (1, 16, 178956960, 1), (1, 16, 178956976, 1), (4, 16, 44739232, 1), (4, 16, 44739248, 1),
    # records of a K = 3 job are as large as the queries; of a K = 1 job a third
    (1, 178956970, 16, 3), (1, 178956971, 16, 3), (64, 2796202, 16, 3), (64, 2796203, 16, 3),
    (1024, 174762, 174768, 1), (1024, 174763, 174768, 1), (1000, 300000, 300000, 3), (1 << 20, 1 << 20, 1 << 20, 3),
]


def test_off32_predicate_matches_the_largest_byte_offset(prog):
    args = [str(v) for s in SHAPES for v in s]
    r = subprocess.run([prog, "off32"] + args, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    got = [int(x) for x in r.stdout.split()]
    assert len(got) == len(SHAPES)
    want = []
    for B, P1, Ppad, K in SHAPES:
        big = _largest_byte_offset(B, P1, Ppad, K)
        # a frame base is formed for frames 0 .. B - 1 and a lane offset added to it; the predicate asks that the whole array
        # (largest offset + 4) stays below 2^31
        want.append(1 if big + 4 < (1 << 31) else 0)
    print(list(zip(SHAPES, got, want)))
    assert got == want
    assert 0 in got and 1 in got
