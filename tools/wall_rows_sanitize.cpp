// Host-only: the wall rows of the viscous surface loads (preprocess.hpp: build_wall_rows) built under a sanitizer and checked
// against a per-node recount (no device, no HIP):
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -Iinclude -Img-cfd-app-plain_amd/csrc tools/wall_rows_sanitize.cpp mg-cfd-app-plain_amd/csrc/preprocess.cpp -lpthread -o /tmp/wall_rows_asan && /tmp/wall_rows_asan
// A random graph of argv[1] nodes (default 3000) in a shuffled numbering, a third of them with one to three solid-wall faces, some
// edges doubled; every index the kernels form from the rows is checked against the size of what it indexes, every row against
// the edges that name its node in edge order, and an edge that names a node out of range must throw.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <numeric>
#include <random>
#include <stdexcept>
#include <vector>
#include "mgcfd.h"
#include "preprocess.hpp"
using namespace mgcfd;
#define CHECK(c) do { if (!(c)) { std::printf("FAILED: %s (line %d)\n", #c, __LINE__); return 1; } } while (0)
int main(int argc, char **argv)
{
    const int64_t nel = argc > 1 ? std::atoll(argv[1]) : 3000;
    std::mt19937 rng(7);
    std::uniform_int_distribution<int64_t> node(0, nel - 1);
    std::uniform_real_distribution<double> w(-1.0, 1.0);
    std::vector<mgcfd_edge> in, bnd, far;
    for (int64_t k = 0; k < 4 * nel; k++) {
        const int64_t a = node(rng), b = node(rng);
        if (a == b) continue;
        in.push_back({a, b, w(rng), w(rng), w(rng)});
        if (k % 17 == 0) in.push_back(in.back());
    }
    for (int64_t i = 0; i < nel; i += 3)
        for (int f = 0; f <= int(i % 3 + i % 2); f++) bnd.push_back({-1, (i * 7919) % nel, w(rng), w(rng), w(rng)});
    std::shuffle(bnd.begin(), bnd.end(), rng);
    for (int64_t i = 0; i < nel; i += 5) far.push_back({-2, i, w(rng), w(rng), w(rng)});
    mgcfd_level_desc d{};
    d.nel = nel; d.internal_start = 0; d.n_internal = int64_t(in.size()); d.boundary_start = d.n_internal; d.n_boundary = int64_t(bnd.size());
    d.wall_start = d.boundary_start + d.n_boundary; d.n_wall = int64_t(far.size());
    std::vector<mgcfd_edge> edges = in;
    edges.insert(edges.end(), bnd.begin(), bnd.end());
    edges.insert(edges.end(), far.begin(), far.end());
    d.n_edges = int64_t(edges.size());
    std::vector<int32_t> new_of_old(static_cast<size_t>(nel));
    std::iota(new_of_old.begin(), new_of_old.end(), 0);
    std::shuffle(new_of_old.begin(), new_of_old.end(), rng);

    const WallRows R = build_wall_rows(d, edges, new_of_old);
    const size_t n = R.original.size();
    CHECK(n > 0 && R.node.size() == n && R.int_ptr.size() == n + 1 && R.wall_ptr.size() == n + 1);
    CHECK(R.int_ptr[0] == 0 && R.wall_ptr[0] == 0 && size_t(R.wall_ptr[n]) == bnd.size() && R.wall_edge.size() == bnd.size() && R.wall_of_rec.size() == bnd.size());
    CHECK(R.int_nbr.size() == size_t(R.int_ptr[n]) && R.int_n.size() == 3 * R.int_nbr.size());
    for (size_t k = 0; k < n; k++) {
        CHECK(k == 0 || R.original[k] > R.original[k - 1]);
        CHECK(R.node[k] == new_of_old[size_t(R.original[k])]);
        // the row against the edges that name the node, in edge order
        size_t at = size_t(R.int_ptr[k]);
        for (const mgcfd_edge &e : in) {
            for (int end = 0; end < 2; end++) {
                if ((end == 0 ? e.a : e.b) != R.original[k]) continue;
                const double s = end == 0 ? 1.0 : -1.0;
                CHECK(at < size_t(R.int_ptr[k + 1]));
                CHECK(R.int_nbr[at] == new_of_old[size_t(end == 0 ? e.b : e.a)]);
                CHECK(R.int_n[3 * at] == s * e.x && R.int_n[3 * at + 1] == s * e.y && R.int_n[3 * at + 2] == s * e.z);
                at++;
            }
        }
        CHECK(at == size_t(R.int_ptr[k + 1]));
        size_t wat = size_t(R.wall_ptr[k]);
        for (size_t j = 0; j < bnd.size(); j++) {
            if (bnd[j].b != R.original[k]) continue;
            CHECK(wat < size_t(R.wall_ptr[k + 1]) && R.wall_edge[wat] == int32_t(j) && R.wall_of_rec[j] == int32_t(k));
            wat++;
        }
        CHECK(wat == size_t(R.wall_ptr[k + 1]) && wat > size_t(R.wall_ptr[k]));
    }
    // a level without solid-wall edges: no wall nodes, empty rows
    mgcfd_level_desc none = d;
    none.n_boundary = 0;
    const WallRows E = build_wall_rows(none, edges, new_of_old);
    CHECK(E.original.empty() && E.int_ptr.size() == 1 && E.int_nbr.empty() && E.wall_edge.empty());
    // an edge that names a node out of range
    edges[size_t(d.boundary_start)].b = nel;
    bool thrown = false;
    try { (void)build_wall_rows(d, edges, new_of_old); } catch (const std::invalid_argument &) { thrown = true; }
    CHECK(thrown);
    std::printf("wall rows: %zu wall nodes of %ld, %zu internal incidences, %zu solid-wall edges: clean\n", n, long(nel), R.int_nbr.size(), bnd.size());
    return 0;
}
