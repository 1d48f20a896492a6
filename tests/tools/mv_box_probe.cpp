// mv_box_probe.cpp -- stand-alone CPU program around csrc/mv_box.h (tests/test_mv_box_cpu.py compiles and runs it; never part of the library).
// stdin:  nv inv_sb Rl[0..8] mvx mvy mvz n      then n lines  wx wy wz size      (floats as C99 hex literals: exact)
// stdout: per particle "hit lox loy loz hix hiy hiz", then "union empty lox loy loz hix hiy hiz" after a pack / unpack round trip.
#include <stdio.h>

#include "mv_box.h"

int main()
{
    int nv, n;
    float inv_sb, Rl[9], mv[3];
    if (scanf("%d %f", &nv, &inv_sb) != 2) return 2;
    for (float& r : Rl) if (scanf("%f", &r) != 1) return 2;
    if (scanf("%f %f %f %d", &mv[0], &mv[1], &mv[2], &n) != 4) return 2;
    MvBox acc = mv_box_empty();
    for (int i = 0; i < n; ++i) {
        float w[4];
        if (scanf("%f %f %f %f", &w[0], &w[1], &w[2], &w[3]) != 4) return 2;
        MvBox b;
        const bool hit = mv_box_of_particle(w[0], w[1], w[2], w[3], mv[0], mv[1], mv[2], Rl, inv_sb, nv, b);
        if (hit) mv_box_union(acc, b);
        printf("%d %d %d %d %d %d %d\n", hit ? 1 : 0, b.lo[0], b.lo[1], b.lo[2], b.hi[0], b.hi[1], b.hi[2]);
    }
    uint32_t x, y;
    mv_box_pack(acc, x, y);
    const MvBox u = mv_box_unpack(x, y);
    printf("union %d %d %d %d %d %d %d\n", mv_box_is_empty(u) ? 1 : 0, u.lo[0], u.lo[1], u.lo[2], u.hi[0], u.hi[1], u.hi[2]);
    return 0;
}
