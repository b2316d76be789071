// Host-only: the wall areas of the heat-flux wall (preprocess.hpp: wall_areas) computed under a sanitizer and checked against a
// per-node recount (no device, no HIP):
//   g++ -O1 -g -std=c++17 -ffp-contract=off -fsanitize=address,undefined -Iinclude -Img-cfd-app-plain_amd/csrc tools/wall_areas_sanitize.cpp mg-cfd-app-plain_amd/csrc/preprocess.cpp -lpthread -o /tmp/wall_areas_asan && /tmp/wall_areas_asan
// A random graph of argv[1] nodes (default 3000) in a shuffled numbering, a third of them with one to three solid-wall faces in
// shuffled order: every area must equal, in bits, the recount over the node's faces in slice order; a level without solid-wall
// edges gives an empty list; a node listed twice, a node out of range, an edge at a node that is not listed and an edge that
// names a node out of range must throw.
#include <algorithm>
#include <cmath>
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
    std::mt19937 rng(11);
    std::uniform_real_distribution<double> w(-1.0, 1.0);
    std::vector<mgcfd_edge> in, bnd;
    for (int64_t i = 0; i + 1 < nel; i++) in.push_back({i, i + 1, w(rng), w(rng), w(rng)});
    for (int64_t i = 0; i < nel; i += 3)
        for (int f = 0; f <= int(i % 3 + i % 2); f++) bnd.push_back({-1, (i * 7919) % nel, w(rng), w(rng), w(rng)});
    std::shuffle(bnd.begin(), bnd.end(), rng);
    mgcfd_level_desc d{};
    d.nel = nel; d.internal_start = 0; d.n_internal = int64_t(in.size()); d.boundary_start = d.n_internal; d.n_boundary = int64_t(bnd.size());
    d.wall_start = d.boundary_start + d.n_boundary; d.n_wall = 0;
    std::vector<mgcfd_edge> edges = in;
    edges.insert(edges.end(), bnd.begin(), bnd.end());
    d.n_edges = int64_t(edges.size());
    std::vector<int32_t> new_of_old(static_cast<size_t>(nel));
    std::iota(new_of_old.begin(), new_of_old.end(), 0);
    std::shuffle(new_of_old.begin(), new_of_old.end(), rng);
    // the wall nodes as the solver lists them: the solver's numbering, ascending, each once
    std::vector<int32_t> nodes;
    for (const mgcfd_edge &e : bnd) nodes.push_back(new_of_old[size_t(e.b)]);
    std::sort(nodes.begin(), nodes.end());
    nodes.erase(std::unique(nodes.begin(), nodes.end()), nodes.end());

    const std::vector<double> area = wall_areas(d, edges, new_of_old, nodes);
    CHECK(area.size() == nodes.size() && !area.empty());
    for (size_t k = 0; k < nodes.size(); k++) {
        double ax = 0.0, ay = 0.0, az = 0.0;
        int faces = 0;
        for (const mgcfd_edge &e : bnd)
            if (new_of_old[size_t(e.b)] == nodes[k]) { ax += e.x; ay += e.y; az += e.z; faces++; }
        const double want = std::sqrt((ax * ax + ay * ay) + az * az);
        CHECK(faces >= 1 && std::memcmp(&want, &area[k], sizeof(double)) == 0);
    }
    // a level without solid-wall edges
    mgcfd_level_desc none = d;
    none.n_boundary = 0;
    CHECK(wall_areas(none, edges, new_of_old, {}).empty());
    // what must be refused
    std::vector<int32_t> twice = nodes; twice.push_back(nodes[0]);
    CHECK(throws([&] { (void)wall_areas(d, edges, new_of_old, twice); }));
    std::vector<int32_t> beyond = nodes; beyond.back() = int32_t(nel);
    CHECK(throws([&] { (void)wall_areas(d, edges, new_of_old, beyond); }));
    std::vector<int32_t> fewer(nodes.begin() + 1, nodes.end());
    CHECK(throws([&] { (void)wall_areas(d, edges, new_of_old, fewer); }));
    edges[size_t(d.boundary_start)].b = nel;
    CHECK(throws([&] { (void)wall_areas(d, edges, new_of_old, nodes); }));
    std::printf("wall areas: %zu wall nodes of %ld, %zu solid-wall edges: clean\n", nodes.size(), long(nel), bnd.size());
    return 0;
}
