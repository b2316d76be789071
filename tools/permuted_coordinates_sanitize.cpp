// Host-only: the coordinates of the corrected face gradient (preprocess.hpp: permuted_coordinates) laid out under a sanitizer and
// checked against a per-node recount (no device, no HIP):
//   g++ -O1 -g -std=c++17 -ffp-contract=off -fsanitize=address,undefined -Iinclude -Img-cfd-app-plain_amd/csrc tools/permuted_coordinates_sanitize.cpp mg-cfd-app-plain_amd/csrc/preprocess.cpp -lpthread -o /tmp/permuted_coordinates_asan && /tmp/permuted_coordinates_asan
// argv[1] nodes (default 3000) in a shuffled numbering, the stride the next multiple of 256: field c of node n must hold, in
// bits, coordinate c of the node's original id, every pad lane +0.0; an empty level gives a stride of zeros; a stride below nel,
// coordinates of another size, a numbering that is too short and a numbering that names a node out of range must throw.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <numeric>
#include <random>
#include <stdexcept>
#include <vector>
#include "mgcfd.h"
#include "preprocess.hpp"
using namespace mgcfd;
#define CHECK(c) do { if (!(c)) { std::printf("FAILED: %s (line %d)\n", #c, __LINE__); return 1; } } while (0)
template <typename F> static bool throws(F &&f)
{
    try { f(); } catch (const std::invalid_argument &) { return true; }
    return false;
}
int main(int argc, char **argv)
{
    const int64_t nel = argc > 1 ? std::atoll(argv[1]) : 3000;
    const int64_t stride = (nel + 255) / 256 * 256;
    std::mt19937 rng(13);
    std::uniform_real_distribution<double> w(-1.0, 1.0);
    std::vector<double> coords(3 * static_cast<size_t>(nel));
    for (double &x : coords) x = w(rng);
    std::vector<int32_t> old_of_new(static_cast<size_t>(nel));
    std::iota(old_of_new.begin(), old_of_new.end(), 0);
    std::shuffle(old_of_new.begin(), old_of_new.end(), rng);

    const std::vector<double> x = permuted_coordinates(coords, old_of_new, nel, stride);
    CHECK(x.size() == 3 * static_cast<size_t>(stride));
    const double zero = 0.0;
    for (int c = 0; c < 3; c++)
        for (int64_t n = 0; n < stride; n++) {
            const double &got = x[static_cast<size_t>(c * stride + n)];
            const double &want = n < nel ? coords[3 * static_cast<size_t>(old_of_new[static_cast<size_t>(n)]) + static_cast<size_t>(c)] : zero;
            CHECK(std::memcmp(&got, &want, sizeof(double)) == 0);
        }
    // an empty level: its pad lanes alone
    const std::vector<double> pad = permuted_coordinates({}, {}, 0, 256);
    CHECK(pad.size() == 768 && std::all_of(pad.begin(), pad.end(), [](double v) { return v == 0.0 && !std::signbit(v); }));
    // a numbering longer than the level is read up to nel only
    std::vector<int32_t> longer = old_of_new; longer.push_back(-5);
    CHECK(permuted_coordinates(coords, longer, nel, stride) == x);
    // what must be refused
    CHECK(throws([&] { (void)permuted_coordinates(coords, old_of_new, nel, nel - 1); }));
    CHECK(throws([&] { (void)permuted_coordinates(coords, old_of_new, -1, stride); }));
    std::vector<double> fewer(coords.begin(), coords.end() - 1);
    CHECK(throws([&] { (void)permuted_coordinates(fewer, old_of_new, nel, stride); }));
    std::vector<int32_t> shorter(old_of_new.begin(), old_of_new.end() - 1);
    CHECK(throws([&] { (void)permuted_coordinates(coords, shorter, nel, stride); }));
    std::vector<int32_t> beyond = old_of_new; beyond[beyond.size() / 2] = static_cast<int32_t>(nel);
    CHECK(throws([&] { (void)permuted_coordinates(coords, beyond, nel, stride); }));
    beyond[beyond.size() / 2] = -1;
    CHECK(throws([&] { (void)permuted_coordinates(coords, beyond, nel, stride); }));
    std::printf("permuted coordinates: %ld nodes in a stride of %ld: clean\n", long(nel), long(stride));
    return 0;
}
