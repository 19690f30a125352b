// The argument checks of the pfg_seq_* entry points (csrc/pfg_seq_checks.hpp) in a host program of their own: built with
// -fsanitize=address,undefined by tests/test_seq_host.py and run there.  Prints "seq checks ok" and returns 0, or says which
// expectation failed.
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

#include "pfg_seq_checks.hpp"

static int failures = 0;

static void expect(int got, int want, const char *what) {
    if (got != want) {
        std::printf("%s: got %d, want %d\n", what, got, want);
        ++failures;
    }
}

int main() {
    using namespace pfg_seq;
    std::vector<double> a(8), b(8);
    const void *four[] = {a.data(), b.data(), a.data(), b.data()};
    const void *hole[] = {a.data(), nullptr, a.data(), b.data()};

    expect(check_rows(2, 1, four, 4, a.data(), b.data()), OK, "smallest population");
    expect(check_rows(kMaxB, 1 << 20, four, 4, a.data(), b.data()), OK, "largest population at 2^40 doubles");
    expect(check_rows(kMaxB, (1 << 20) + 1, four, 4, a.data(), b.data()), BAD_ROW, "past 2^40 doubles");
    expect(check_rows(2, std::numeric_limits<int64_t>::max(), four, 4, a.data(), b.data()), BAD_ROW, "row_doubles = INT64_MAX");
    expect(check_rows(2, 0, four, 4, a.data(), b.data()), BAD_ROW, "row_doubles = 0");
    expect(check_rows(2, -3, four, 4, a.data(), b.data()), BAD_ROW, "row_doubles < 0");
    expect(check_rows(1, 4, four, 4, a.data(), b.data()), BAD_B, "B = 1");
    expect(check_rows(0, 4, four, 4, a.data(), b.data()), BAD_B, "B = 0");
    expect(check_rows(std::numeric_limits<int>::min(), 4, four, 4, a.data(), b.data()), BAD_B, "B = INT_MIN");
    expect(check_rows(kMaxB + 1, 4, four, 4, a.data(), b.data()), BAD_B, "B = 2^20 + 1");
    expect(check_rows(std::numeric_limits<int>::max(), 4, four, 4, a.data(), b.data()), BAD_B, "B = INT_MAX");
    expect(check_rows(2, 4, hole, 4, a.data(), b.data()), NULL_ARGUMENT, "a NULL argument");
    expect(check_rows(2, 4, four, 4, a.data(), a.data()), ALIAS, "the two row arrays alias");
    expect(check_rows(2, 4, four, 0, a.data(), b.data()), OK, "no pointers to check");

    expect(check_reweight(1, 0.5, four, 4), OK, "stride 1");
    expect(check_reweight(0, 1.0, four, 4), OK, "stride 0, target 1");
    expect(check_reweight(8, std::ldexp(1.0, -1000), four, 4), OK, "a tiny target");
    expect(check_reweight(-1, 0.5, four, 4), BAD_STRIDE, "stride < 0");
    expect(check_reweight(std::numeric_limits<int64_t>::min(), 0.5, four, 4), BAD_STRIDE, "stride = INT64_MIN");
    expect(check_reweight(1, 0.0, four, 4), BAD_TARGET, "target 0");
    expect(check_reweight(1, -0.5, four, 4), BAD_TARGET, "target < 0");
    expect(check_reweight(1, std::nextafter(1.0, 2.0), four, 4), BAD_TARGET, "target just above 1");
    expect(check_reweight(1, std::numeric_limits<double>::quiet_NaN(), four, 4), BAD_TARGET, "target NaN");
    expect(check_reweight(1, std::numeric_limits<double>::infinity(), four, 4), BAD_TARGET, "target inf");
    expect(check_reweight(1, 0.5, hole, 4), NULL_ARGUMENT, "reweight: a NULL argument");

    if (failures) return 1;
    std::printf("seq checks ok\n");
    return 0;
}
