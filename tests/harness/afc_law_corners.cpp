// The AFC law (navtex_amd/csrc/nvx_afc_law.h) as a plain host program: tests/test_afc.py builds it with
// -fsanitize=address,undefined and feeds it its table of cases -- one per line: gain_shift max_step range_k min_samples
// contrast_min kc k0 k1 samples b_samples sum_dphi_b sum_dphi_y sum_mf_hi sum_mf_lo want_k2 want_flags, the doubles as
// C99 hexadecimal literals, nan or inf -- and it holds every answer against the restatement's.  Runs on the CPU only.
#include <cstdio>
#include <cstdlib>
#include "nvx_afc_law.h"

int main(int argc, char **argv)
{
    if (argc != 2) { fprintf(stderr, "usage: %s cases.txt\n", argv[0]); return 2; }
    FILE *f = fopen(argv[1], "r");
    if (!f) { perror(argv[1]); return 2; }
    char line[1024];
    long n = 0, bad = 0;
    while (fgets(line, sizeof line, f)) {
        nvx_afc_par p{};
        int k0, k1, want_k2;
        unsigned samples, b_samples, want_flags, flags = 0;
        double sb, sy, hi, lo;
        p.track = 1;
        if (sscanf(line, "%d %d %d %d %la %d %d %d %u %u %la %la %la %la %d %u", &p.gain_shift, &p.max_step, &p.range_k, &p.min_samples,
                   &p.contrast_min, &p.kc, &k0, &k1, &samples, &b_samples, &sb, &sy, &hi, &lo, &want_k2, &want_flags) != 16) {
            fprintf(stderr, "line %ld: not a case: %s", n + 1, line); fclose(f); return 2;
        }
        const int k2 = nvx_afc_step(&p, k0, k1, samples, b_samples, sb, sy, hi, lo, &flags);
        if (k2 != want_k2 || flags != want_flags) {
            if (++bad <= 20) fprintf(stderr, "case %ld: k2 %d flags %u, the restatement has %d and %u: %s", n + 1, k2, flags, want_k2, want_flags, line);
        }
        n++;
    }
    fclose(f);
    if (bad) { printf("afc law: %ld of %ld cases differ\n", bad, n); return 1; }
    printf("afc law corners ok %ld\n", n);
    return 0;
}
