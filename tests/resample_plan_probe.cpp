// Probe of csrc/gdx_resample_plan.h for tests/test_resample_host.py: the header compiles as plain C++17 without HIP.
// One case per input line.  "W N jump repeats" prints the walk: calls, hops, then "r<index>" / "f<from>,<to>" per hop.
// "C from to n abar_0 .. abar_{n-1}" (hexadecimal floats) prints the bits of the forward hop's (a, b).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "gdx_resample_plan.h"

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        char what;
        if (!(in >> what)) return 1;
        if (what == 'W') {
            int N, jump, repeats;
            if (!(in >> N >> jump >> repeats)) return 1;
            const std::vector<gdx::Hop> hops = gdx::resample_walk(N, jump, repeats);
            std::printf("%ld %ld", gdx::resample_calls(N, jump, repeats), gdx::resample_hops(N, jump, repeats));
            for (const gdx::Hop& h : hops) {
                if (h.forward) std::printf(" f%d,%d", h.from, h.to);
                else std::printf(" r%d", h.to);
            }
            std::printf("\n");
        } else if (what == 'C') {
            int from, to, n;
            if (!(in >> from >> to >> n)) return 1;
            std::vector<double> ab(n);
            std::string word;
            for (double& v : ab) { if (!(in >> word)) return 1; v = std::strtod(word.c_str(), nullptr); }
            float a, b;
            gdx::resample_coef(ab.data(), from, to, &a, &b);
            uint32_t ia, ib;
            std::memcpy(&ia, &a, 4);
            std::memcpy(&ib, &b, 4);
            std::printf("%u %u\n", ia, ib);
        } else {
            return 1;
        }
    }
    return 0;
}
