// The launches of a solve from the levels' widths (csrc/prover_key.h
// SolvePlan::launch_runs, a plain host function): prints the runs of the
// levels given on the command line, for tests/test_solve_runs.py to compare
// with tuples written out there.
//   solve_runs [arith+gate ...]   ->  one line "l0 l1 p0 p1 g0 g1 wide" a run
#include "prover_key.h"
#include <cstdio>
#include <cstdlib>

int main(int argc, char **argv) {
    std::vector<uint32_t> widths, gate_widths;
    for (int k = 1; k < argc; k++) {
        char *end = nullptr;
        widths.push_back((uint32_t)strtoul(argv[k], &end, 10));
        gate_widths.push_back(*end == '+' ? (uint32_t)strtoul(end + 1, nullptr, 10) : 0);
    }
    for (const auto &r : pnp::ResidentKey::SolvePlan::launch_runs(widths, gate_widths))
        printf("%u %u %llu %llu %llu %llu %d\n", r.l0, r.l1, (unsigned long long)r.p0, (unsigned long long)r.p1,
               (unsigned long long)r.g0, (unsigned long long)r.g1, (int)r.wide);
    return 0;
}
