// fg_smc_plan.h (fugue_amd/csrc) over cases on stdin, for tests/test_smc_plan_cpu.py (g++, no GPU; once more with -fsanitize=address,undefined).
//   smc_plan_driver variants     the keys of FG_SMC_REJUV_VARIANTS, one per line: score gt
//   smc_plan_driver regions      the arena's regions in carving order, one name per line
//   smc_plan_driver              one line per case of stdin:
//       rejuv N S d n_slots tw has_sstream sstream_kinds sstream_gen jit_state sequential from_run
//           -> rc [score global_tile wpb lds nblk threads try_compiled  key: score gt seq] | rc [wpb lds nblk] (fg_smc_jit_rejuv_shape(S, N)) | name
//       arena N S ess2_doubles
//           -> bytes adapt_reset_off adapt_reset_bytes (off len)*
#include <cstdio>
#include <iostream>
#include <sstream>

#include "../../fugue_amd/csrc/fg_smc_plan.h"

int main(int argc, char **argv) {
    if (argc == 2 && std::string(argv[1]) == "variants") {
#define FG_PRINT_KEY(SCORE, GT) std::printf("%d %d\n", SCORE, (int)GT);
        FG_SMC_REJUV_VARIANTS(FG_PRINT_KEY)
        return 0;
    }
    if (argc == 2 && std::string(argv[1]) == "regions") {
#define FG_PRINT_REGION(name, bytes) std::printf("%s\n", #name);
        FG_SMC_REGIONS(FG_PRINT_REGION)
        return 0;
    }
    if (argc != 1) return 2;
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream s(line);
        std::string what;
        s >> what;
        if (what == "arena") {
            long long N; int S; size_t ess2;
            s >> N >> S >> ess2;
            if (!s) return 3;
            const FgSmcArena A = fg_smc_arena_layout(N, S, ess2);
            std::cout << A.bytes << ' ' << A.adapt_reset_off << ' ' << A.adapt_reset_bytes;
            for (int r = 0; r < FG_SMC_N_REGIONS; ++r) std::cout << ' ' << A.off[r] << ' ' << A.len[r];
            std::cout << '\n';
        } else if (what == "rejuv") {
            FgSmcRejuvIn in{};
            int n_slots, flag[4];
            s >> in.N >> in.S >> in.d >> n_slots >> in.tw >> flag[0] >> in.sstream_kinds >> flag[1] >> in.jit_state >> flag[2] >> flag[3];
            if (!s) return 3;
            in.lds_score = (size_t)n_slots * in.tw * sizeof(double);
            in.has_sstream = flag[0]; in.sstream_gen = flag[1]; in.sequential = flag[2]; in.from_run = flag[3];
            FgSmcRejuvPlan p;
            const int rc = fg_smc_rejuv_plan(in, &p);
            std::cout << rc;
            if (rc == FG_OK)
                std::cout << ' ' << p.score << ' ' << p.global_tile << ' ' << p.wpb << ' ' << p.lds << ' ' << p.nblk << ' ' << p.threads << ' ' << p.try_compiled << ' '
                          << p.key.score << ' ' << p.key.gt << ' ' << p.key.seq;
            FgSmcJitShape sh;
            const int jrc = fg_smc_jit_rejuv_shape(in.S, in.N, &sh);
            std::cout << " | " << jrc;
            if (jrc == FG_OK) std::cout << ' ' << sh.wpb << ' ' << sh.lds << ' ' << sh.nblk;
            std::cout << " | " << (rc == FG_OK ? p.name : std::string("-")) << '\n';
        } else return 3;
    }
    return 0;
}
