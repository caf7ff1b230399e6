// Private to the library, host only: what a host twin needs of a mode's tables, kept for the last geometry asked for, so that a sweep over
// frames builds the tables once. Not part of the ABI.
#pragma once
#include <memory>
#include <mutex>

#include "tables.hpp"

extern "C" const unsigned char mgpu_ldpc_blob[];
extern "C" const unsigned long mgpu_ldpc_blob_size;

namespace mgpu_detail {

template <typename G> struct GeometrySlot {
    std::mutex mutex;
    int cfg = -1;
    mgpu::ExplicitParams xp;
    std::shared_ptr<const G> g;
};
template <typename G> GeometrySlot<G>& geometry_slot() {
    static GeometrySlot<G> slot;
    return slot;
}

// G = make(the tables of (cfg, xp)): the one G's slot holds where that is its geometry, else built (build_mode_tables throws on a bad cfg)
// and kept there. One slot per G, on purpose: the ladder's twins normalise ls_window before they ask and the others do not, so one shared
// slot would be rebuilt whenever a caller alternates between twins. A caller keeps its G alive by the pointer, whatever the slot holds by
// then.
template <typename G, typename Make>
std::shared_ptr<const G> cached_geometry(int cfg, const mgpu::ExplicitParams& xp, Make&& make) {
    GeometrySlot<G>& slot = geometry_slot<G>();
    std::lock_guard<std::mutex> lock(slot.mutex);
    if (slot.g && slot.cfg == cfg && slot.xp == xp) return slot.g;
    std::shared_ptr<const G> g = std::make_shared<const G>(make(mgpu::build_mode_tables(cfg, 0, mgpu_ldpc_blob, mgpu_ldpc_blob_size, xp)));
    slot.cfg = cfg; slot.xp = xp; slot.g = g;
    return g;
}

}  // namespace mgpu_detail
