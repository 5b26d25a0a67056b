// Stand-alone driver of the two host functions behind the two-head form of the fused QKV + attention kernel, built by tests/test_qkv_pair_host.py with the
// host compiler alone (plain and with -fsanitize=address,undefined):
//
//     qkv_pair_main rows D      the pair-ordered row (csrc/tld_refresh_math.h: qkv_pair_row) of every row n = part * D + head * 64 + r of a [3 D][D] QKV
//                               weight, 3 D numbers on one line
//     qkv_pair_main plan        csrc/tld_qkv_pair_plan.h: plan_qkv_pair -- first "ratio NUM DEN", then one line "HEADS CUS 0110..." per (heads, CU count) in
//                               {6, 12, 16} x {256, 304} with one digit per sample count 1 .. 512
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "tld_qkv_pair_plan.h"
#include "tld_refresh_math.h"

int main(int argc, char** argv) {
    if (argc == 3 && !strcmp(argv[1], "rows")) {
        const int d = atoi(argv[2]);
        if (d < 64 || d % 64) return 2;
        for (int n = 0; n < 3 * d; ++n) {
            const int part = n / d, head = (n - part * d) >> 6, r = n & 63;
            printf("%d%c", tld::qkv_pair_row(part, head, r), n + 1 < 3 * d ? ' ' : '\n');
        }
        return 0;
    }
    if (argc == 2 && !strcmp(argv[1], "plan")) {
        printf("ratio %ld %ld\n", tld::kQkvPairCostNum, tld::kQkvPairCostDen);
        const int heads[3] = {6, 12, 16}, cus[2] = {256, 304};
        for (int h : heads)
            for (int c : cus) {
                printf("%d %d ", h, c);
                for (int s = 1; s <= 512; ++s) putchar(tld::plan_qkv_pair(s, h, c) ? '1' : '0');
                putchar('\n');
            }
        return 0;
    }
    fprintf(stderr, "usage: qkv_pair_main rows D | plan\n");
    return 2;
}
