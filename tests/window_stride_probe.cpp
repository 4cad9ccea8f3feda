// Probe of csrc/gdx_window_stride.h for tests/test_parallel_host.py: the header compiles as plain C++17 without HIP.
// One case per input line: batch n first_index num_steps, then num_steps thresholds, then n * batch errors ("nan" allowed);
// prints the stride.
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "gdx_window_stride.h"

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        int batch, n, first, steps;
        if (!(in >> batch >> n >> first >> steps)) return 1;
        std::vector<double> thr(steps), err((size_t)n * batch);
        std::string word;
        for (double& v : thr) { if (!(in >> word)) return 1; v = std::strtod(word.c_str(), nullptr); }
        for (double& v : err) { if (!(in >> word)) return 1; v = std::strtod(word.c_str(), nullptr); }
        std::printf("%d\n", gdx::window_stride(err.data(), batch, n, thr.data(), first));
    }
    return 0;
}
