// Host driver for csrc/tld_tail_fold_math.h: the folded out_proj operand, element by element as refresh_tail_fold_kernel builds it.
//   tail_fold_main pd d hid in.bin out.bin
// in.bin:  fp32 Wout [pd][d] | Wd [d][hid] | bd [d] | bo [pd]
// out.bin: fp32 W' [pd][hid] | b' [pd] | uint16 image [2][pdp][d + hid] (hi plane, lo plane; rows >= pd zero)
// tests/test_tail_fold_host.py holds the output bit for bit against a numpy float64 restatement, and runs this program once under
// -fsanitize=address,undefined.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "tld_tail_fold_math.h"

int main(int argc, char** argv) {
    if (argc != 6) { fprintf(stderr, "usage: tail_fold_main pd d hid in.bin out.bin\n"); return 2; }
    const int pd = atoi(argv[1]), d = atoi(argv[2]), hid = atoi(argv[3]);
    if (pd <= 0 || d <= 0 || hid <= 0) return 2;
    const size_t n_in = (size_t)pd * d + (size_t)d * hid + (size_t)d + (size_t)pd;
    std::vector<float> in(n_in);
    FILE* f = fopen(argv[4], "rb");
    if (!f || fread(in.data(), 4, n_in, f) != n_in) { fprintf(stderr, "short input\n"); return 2; }
    fclose(f);
    const float *wout = in.data(), *wd = wout + (size_t)pd * d, *bd = wd + (size_t)d * hid, *bo = bd + d;
    const int pdp = tld::tail_fold_padded_rows(pd), K = d + hid;
    std::vector<float> wf((size_t)pd * hid), bf((size_t)pd);
    std::vector<uint16_t> img((size_t)2 * pdp * K, 0);
    for (int r = 0; r < pd; ++r) {
        for (int j = 0; j < hid; ++j) wf[(size_t)r * hid + j] = tld::tail_fold_weight(wout + (size_t)r * d, wd, d, hid, j);
        bf[(size_t)r] = tld::tail_fold_bias(wout + (size_t)r * d, bd, bo[r], d);
        for (int k = 0; k < K; ++k) {
            const float w = k < d ? wout[(size_t)r * d + k] : wf[(size_t)r * hid + (k - d)];
            tld::tail_fold_split(w, &img[(size_t)r * K + k], &img[((size_t)pdp + r) * K + k]);
        }
    }
    f = fopen(argv[5], "wb");
    if (!f) return 2;
    const bool ok = fwrite(wf.data(), 4, wf.size(), f) == wf.size() && fwrite(bf.data(), 4, bf.size(), f) == bf.size() &&
                    fwrite(img.data(), 2, img.size(), f) == img.size();
    fclose(f);
    return ok ? 0 : 1;
}
