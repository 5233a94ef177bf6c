"""The chunk arithmetic of csrc/row_store.h, checked exhaustively on the host: a stand-alone program compiled with the
host compiler against the header walks every (elements per chunk, misalignment, row length, chunks per workgroup) and
checks the properties the chunked kernels rely on.  Everything is derived: no tolerance."""
import os
import subprocess
import tempfile


PROGRAM = r"""
#include <stdio.h>
#include <stdlib.h>
#include "row_store.h"

#define CHECK(cond) do { if (!(cond)) { \
    printf("line %d: %s  (E %d s %d F %d G %d c %d)\n", __LINE__, #cond, E, s, F, G, c); return 1; } } while (0)

template <typename I> static int run(long *cases)
{
    static char arena[64] __attribute__((aligned(16)));
    const int Es[2] = {16, 4}, Gs[4] = {1, 2, 3, 1024};
    for (int ei = 0; ei < 2; ei++) {
        const int E = Es[ei];
        for (int s = 0; s < E; s++)
            for (int F = 1; F <= 3 * E + 2; F++) {
                int G = 0, c = 0;
                /* the misalignment of a base that lies s elements above an aligned address, for several such addresses */
                for (int a = 0; a < 48; a += 16) CHECK(mg_row_misalign(arena + a + s * (16 / E), E) == s);
                const I count = mg_row_chunks<I>((I)F, E), exact = mg_row_chunks_at<I>(s, (I)F, E);
                /* the old closed forms */
                CHECK(count == (E == 16 ? ((I)F + 15 + 15) / 16 : ((I)F + 3 + 3) / 4));
                if (E == 16) CHECK(exact == ((s + F + 15) >> 4));
                CHECK(exact <= count && exact == mg_row_chunks_at<I>(s, (I)F, E));
                /* the chunks' own ranges partition [0, F) in order, over the host-side count */
                I next = 0;
                for (c = 0; c < (int)count; c++) {
                    const mg_row_chunk_t<I> k = mg_row_chunk<I>(s, (I)F, (I)c, E);
                    CHECK(k.p == (I)E * c - s && k.p > -(I)E);
                    if (k.lo < k.hi) {
                        CHECK(k.lo == next && k.hi <= F && k.lo >= k.p && k.hi <= k.p + E);
                        next = k.hi;
                    } else {
                        CHECK(c >= (int)exact && !k.whole);      /* only the spare chunk of the any-base count is empty */
                    }
                    if (k.whole) {                               /* inside the row, one aligned 16-byte store */
                        CHECK(k.p >= 0 && k.p + E <= F && k.lo == k.p && k.hi == k.p + E);
                        CHECK(((s + k.p) % E) == 0);
                        CHECK(((uintptr_t)(arena + (s + k.p) * (16 / E)) & 15) == 0);
                    } else if (k.lo < k.hi) {
                        CHECK(k.p < 0 || k.p + E > F);
                    }
                }
                CHECK(next == F);
                for (c = (int)count; c < (int)count + 3; c++) {  /* no chunk beyond the count has elements */
                    const mg_row_chunk_t<I> k = mg_row_chunk<I>(s, (I)F, (I)c, E);
                    CHECK(k.lo >= k.hi && !k.whole);
                }
                /* the workgroup spans partition [0, F) too, and hold exactly their chunks' elements */
                for (int gi = 0; gi < 4; gi++) {
                    G = Gs[gi];
                    const I groups = (count + G - 1) / G;        /* what the launches provide */
                    I at = 0;
                    for (I b = 0; b < groups; b++) {
                        const mg_row_span_t<I> g = mg_row_span<I>(s, (I)F, b, (I)G, E);
                        c = (int)b;
                        CHECK(g.c0 == b * G);
                        if (g.c0 >= g.c1) continue;              /* a workgroup without chunks stores nothing */
                        CHECK(g.c1 <= g.c0 + G && g.c1 <= exact && g.p_lo == at && g.p_lo < g.p_hi && g.p_hi <= F);
                        CHECK(g.p_lo == mg_row_chunk<I>(s, (I)F, g.c0, E).lo && g.p_hi == mg_row_chunk<I>(s, (I)F, g.c1 - 1, E).hi);
                        at = g.p_hi;
                    }
                    CHECK(at == F);
                    ++*cases;
                }
            }
    }
    return 0;
}

int main(void)
{
    long cases = 0;
    if (run<int>(&cases) || run<int64_t>(&cases)) return 1;
    printf("ok %ld\n", cases);
    return 0;
}
"""


def test_chunk_arithmetic_exhaustively_on_the_host():
    import twoarmy_amd
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "row_store_check.cpp"), os.path.join(d, "row_store_check")
        with open(src, "w") as f:
            f.write(PROGRAM)
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", twoarmy_amd._lib.CSRC_DIR, src,
                               "-o", exe])
        r = subprocess.run([exe], stdout=subprocess.PIPE, universal_newlines=True)
    assert r.returncode == 0, r.stdout
    # E in {16, 4} x s in [0, E) x F in 1..3E+2 x 4 workgroup sizes, for both index types
    want = 2 * 4 * sum(E * (3 * E + 2) for E in (16, 4))
    assert r.stdout.split() == ["ok", str(want)], r.stdout
