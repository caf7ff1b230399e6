// The host twins' geometry cache (mercury_amd/csrc/geometry_cache.hpp) as a stand-alone program for the sanitizers: built from this file,
// mercury_amd/csrc/tables.cpp and the LDPC table blob with -fsanitize=address,undefined, and again with -fsanitize=thread, and run on the
// CPU (tests/test_stage_plumbing_host.py). One thread first checks the slot's rule - the same geometry twice is one object, another one
// replaces it, a G handed out stays alive and unchanged - then four threads alternate two geometries, so that every call finds the slot
// holding the other one as often as not, and check that what they get is what they asked for.
#include <cstdio>
#include <memory>
#include <thread>
#include <vector>

#include "check.hpp"
#include "geometry_cache.hpp"

namespace {

struct Toy {
    int cfg = 0, Nsymb = 0, Dy = 0, nPilots = 0;
    std::vector<uint8_t> cell_type;
};

std::shared_ptr<const Toy> toy(int cfg, const mgpu::ExplicitParams& xp) {
    return mgpu_detail::cached_geometry<Toy>(cfg, xp, [](const mgpu::ModeTables& t) { return Toy{t.cfg, t.Nsymb, t.xp.Dy, t.nPilots, t.cell_type}; });
}

bool is_geometry(const Toy& g, int cfg, const mgpu::ExplicitParams& xp) {
    if (g.cfg != cfg || g.Nsymb != xp.Nsymb || g.Dy != xp.Dy || g.cell_type.size() != size_t(xp.Nsymb) * 50) return false;
    int pilots = 0;
    for (uint8_t c : g.cell_type) pilots += c != 0;
    return pilots == g.nPilots && pilots > 0;
}

}  // namespace

int main() {
    const int cfg = 13;
    mgpu::ExplicitParams a, b;
    a.Nsymb = 8;
    b.Nsymb = 8; b.Dy = 5;
    CHECK(a == a && !(a == b));

    const std::shared_ptr<const Toy> first = toy(cfg, a);
    CHECK(is_geometry(*first, cfg, a));
    CHECK(toy(cfg, a) == first);                        // kept
    const std::shared_ptr<const Toy> other = toy(cfg, b);
    CHECK(other != first && is_geometry(*other, cfg, b) && other->nPilots != first->nPilots);
    CHECK(is_geometry(*first, cfg, a));                 // what was handed out is the caller's
    CHECK(toy(cfg, a) != first && toy(cfg, a) == toy(cfg, a));
    bool threw = false;
    try {
        toy(-5, a);
    } catch (const std::exception&) { threw = true; }
    CHECK(threw && is_geometry(*toy(cfg, a), cfg, a));  // a refused cfg leaves the slot usable

    int bad[4] = {0, 0, 0, 0};
    std::vector<std::thread> threads;
    for (int t = 0; t < 4; ++t)
        threads.emplace_back([&, t] {
            for (int i = 0; i < 12; ++i) {
                const mgpu::ExplicitParams& want = ((i + t) & 1) ? b : a;
                const std::shared_ptr<const Toy> g = toy(cfg, want);
                if (!is_geometry(*g, cfg, want)) ++bad[t];
            }
        });
    for (auto& th : threads) th.join();
    CHECK(bad[0] + bad[1] + bad[2] + bad[3] == 0);
    if (failures) return 1;
    std::printf("geometry cache: clean\n");
    return 0;
}
