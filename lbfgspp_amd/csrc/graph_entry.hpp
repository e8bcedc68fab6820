// lbfgspp_amd/csrc/graph_entry.hpp -- one entry of a graph objective's incidence list, shared by the translation unit that
// builds the list (graph_topology.hip) and the kernels that walk it (graph_kernels.cuh, compiled at run time).
#pragma once
#include <stdint.h>

namespace lbfgsx {

// node v's entries are inc[off[v] .. off[v+1]) in ascending edge index e.  v is end `side` of edge e (0: ei[e], 1: ej[e]),
// `other` is the edge's other end, es = (e << 1) | side.  8 bytes: one load per entry.
struct alignas(8) GraphEntry
{
    int32_t other;
    uint32_t es;
};

}  // namespace lbfgsx
