// Prints the plans of csrc/gdx_call_plan.h for the cases on stdin (tests/test_call_plan_host.py); plain C++17, no HIP.
//   M n t0 .. t(n-1)                                                              the timestep map of the cases that follow
//   L lo hi every lc_every mode num_steps first_index k_base last_index two_calls   plan_loop
//   U lo hi every lc_every mode first count dir                                     plan_unnumbered
// One line per case: "bad" where plan_loop refuses, else the position of the block's first call in the plan, whether the block
// begins with a reuse, and the block's own calls from there on as idx,mode,lc,K.
#include "gdx_call_plan.h"

#include <iostream>
#include <string>

int main() {
    std::ios::sync_with_stdio(false);
    std::vector<int64_t> map;
    std::string out;
    char tag;
    while (std::cin >> tag) {
        if (tag == 'M') {
            size_t n;
            std::cin >> n;
            map.assign(n, 0);
            map.shrink_to_fit();
            for (auto& t : map) std::cin >> t;
            continue;
        }
        gdx::PlanRule r;
        int mode;
        std::cin >> r.guide_lo >> r.guide_hi >> r.guide_every >> r.lc_every >> mode;
        gdx::CallPlan p;
        size_t begin = 0;
        if (tag == 'L') {
            gdx::CallSeq q{mode, map.data()};
            std::cin >> q.num_steps >> q.first_index >> q.k_base >> q.last_index >> q.two_calls;
            if (!gdx::plan_loop(r, q, &p)) {
                out += "bad\n";
                continue;
            }
            begin = &p.step(q.k_base) - p.calls.data();
        } else {
            int first, count, dir;
            std::cin >> first >> count >> dir;
            p = gdx::plan_unnumbered(r, mode, map.data(), first, count, dir);
        }
        out += std::to_string(begin) + " " + std::to_string(p.begins_with_reuse());
        for (size_t i = begin; i < p.calls.size(); ++i) {
            const gdx::PlannedCall& e = p.calls[i];
            out += " " + std::to_string(e.idx) + "," + std::to_string(e.mode) + "," + std::to_string(e.lc) + "," + std::to_string(e.K);
        }
        out += "\n";
    }
    std::cout << out;
    return 0;
}
