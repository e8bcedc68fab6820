// lbfgspp_amd/csrc/form_table.hpp -- the forms of a compiled objective (include/lbfgsx.h: LBFGSX_FORM_*), one row each of what
// the host says about a form: its names in messages and entry points, and for a LATTICE form -- one on a regular array: grid,
// volume, the two periodic ones, grid field, grid stencil -- the rules its shape and mask obey.  liblbfgsx.so (jit_objective.hip)
// and liblbfgsx_solver.so (solver_capi.cpp) both refuse by these rows, in the same words.  Plain C++: nothing of HIP in here.
#pragma once
#include <cstdint>
#include <string>

#include "../../include/lbfgsx.h"

namespace lbfgsx {

struct FormRow
{
    const char* name;             // in messages
    const char* suffix;           // of lbfgsx_objective_compile, _source, _bind and lbfgsx_solver_minimize for this form
    const char* bound_with;       // what lbfgsx_objective_bind says the form is bound with; null: it binds it
    const char* bind_suffix;      // of the calls that bind and minimise it, where they are another form's; null: suffix
    const char* minimised_with;   // what lbfgsx_solver_minimize_obj says in place of bound_with; null: the same
    // a lattice form (axes != 0)
    int axes;                     // 2: rows x cols; 3: slabs x rows x cols
    int min_extent;               // of every axis
    const char* extent_rule;      // the sentence of an extent below it
    int mask_hi;                  // the periodic mask lies in 0 .. mask_hi; -1: the form takes no mask
    const char* mask_rule;        // the sentence of a mask outside
    bool times_D;                 // n is the extents' product times the handle's D
};
#define LBFGSX_GRID_EXTENT "a grid has at least 2 rows and 2 columns (rows >= 2, cols >= 2)"
#define LBFGSX_VOLUME_EXTENT "a volume has at least 2 slabs, 2 rows and 2 columns (slabs >= 2, rows >= 2, cols >= 2)"
#define LBFGSX_GRID_MASK "the mask has bit 0 for the column direction and bit 1 for the row direction (0 .. 3)"
#define LBFGSX_LIST_FORM 0, 0, nullptr, -1, nullptr, false
// by LBFGSX_FORM_*
inline constexpr FormRow kFormRows[14] = {
    {"term objective", "", nullptr, nullptr, nullptr, LBFGSX_LIST_FORM},
    {"chain objective", "_chain", nullptr, nullptr, nullptr, LBFGSX_LIST_FORM},
    {"grid objective", "_grid", "shape", nullptr, nullptr, 2, 2, LBFGSX_GRID_EXTENT, -1, nullptr, false},
    {"graph objective", "_graph", "edges", nullptr, nullptr, LBFGSX_LIST_FORM},
    {"mesh objective", "_mesh", "elements", nullptr, nullptr, LBFGSX_LIST_FORM},
    {"linear-model objective", "_linear", "matrix", nullptr, nullptr, LBFGSX_LIST_FORM},
    {"multi-output linear-model objective", "_linear_multi", "matrix", "_linear", nullptr, LBFGSX_LIST_FORM},
    {"dense linear-model objective", "_dense", "matrix", nullptr, nullptr, LBFGSX_LIST_FORM},
    {"graph-regularised linear-model objective", "_linear_graph", "matrix and edges", nullptr, nullptr, LBFGSX_LIST_FORM},
    {"volume objective", "_volume", "shape", nullptr, nullptr, 3, 2, LBFGSX_VOLUME_EXTENT, -1, nullptr, false},
    {"periodic grid objective", "_grid_periodic", "shape and mask", nullptr, nullptr, 2, 2, LBFGSX_GRID_EXTENT, 3, LBFGSX_GRID_MASK,
     false},
    {"periodic volume objective", "_volume_periodic", "shape and mask", nullptr, nullptr, 3, 2, LBFGSX_VOLUME_EXTENT, 7,
     "the mask has bit 0 for the column, bit 1 for the row and bit 2 for the slab direction (0 .. 7)", false},
    {"grid field objective", "_grid_field", "shape, mask and D", nullptr, "shape and mask", 2, 2, LBFGSX_GRID_EXTENT, 3,
     LBFGSX_GRID_MASK, true},
    {"grid stencil objective", "_grid_stencil", "shape and mask", nullptr, nullptr, 2, 3,
     "a 3x3 patch needs at least 3 rows and 3 columns (rows >= 3, cols >= 3)", 3, LBFGSX_GRID_MASK, false}};
#undef LBFGSX_GRID_EXTENT
#undef LBFGSX_VOLUME_EXTENT
#undef LBFGSX_GRID_MASK
#undef LBFGSX_LIST_FORM

// what the call without the form's arguments says of a form that has some: lbfgsx_objective_bind, or lbfgsx_solver_minimize_obj
inline std::string unshaped_refusal(int form, bool minimise)
{
    const FormRow& r = kFormRows[form];
    const char* suffix = r.bind_suffix ? r.bind_suffix : r.suffix;
    if (minimise)
        return std::string("a ") + r.name + " is minimised with its " + (r.minimised_with ? r.minimised_with : r.bound_with) +
               ": lbfgsx_solver_minimize" + suffix;
    return std::string("a ") + r.name + " is bound with its " + r.bound_with + ": lbfgsx_objective_bind" + suffix;
}

// ---- a lattice form's row applied to a request
enum LatticeRule { LATTICE_OK = 0, LATTICE_EXTENT, LATTICE_OVERFLOW, LATTICE_MASK };

// the first rule the request fails, in this order: an extent below the minimum, a product (times D where the form says so)
// that overflows, a mask outside its range.  n: the product, once the first two hold.  slabs is not looked at on two axes, nor
// periodic by a form without a mask.  The two callers differ on purpose: the solver's entry point has no n yet and reports
// the overflow; the bind call has one and reports overflow as a product that is not n, ahead of the mask
inline LatticeRule lattice_check(int form, int D, int64_t slabs, int64_t rows, int64_t cols, int periodic, long long* n)
{
    const FormRow& r = kFormRows[form];
    if (rows < r.min_extent || cols < r.min_extent || (r.axes == 3 && slabs < r.min_extent))
        return LATTICE_EXTENT;
    long long prod = 0;
    if (__builtin_mul_overflow((long long) rows, (long long) cols, &prod) ||
        (r.axes == 3 && __builtin_mul_overflow(prod, (long long) slabs, &prod)) ||
        (r.times_D && __builtin_mul_overflow(prod, (long long) D, &prod)))
        return LATTICE_OVERFLOW;
    *n = prod;
    return r.mask_hi >= 0 && (periodic < 0 || periodic > r.mask_hi) ? LATTICE_MASK : LATTICE_OK;
}

// "slabs = 2, rows = 3, cols = 4", with ", D = 2" where D enters the product
inline std::string lattice_shape(int form, int D, int64_t slabs, int64_t rows, int64_t cols)
{
    const FormRow& r = kFormRows[form];
    return (r.axes == 3 ? "slabs = " + std::to_string(slabs) + ", " : std::string()) + "rows = " + std::to_string(rows) +
           ", cols = " + std::to_string(cols) + (r.times_D ? ", D = " + std::to_string(D) : std::string());
}

// the message of a failed rule; an overflow in the words of the solver's entry point
inline std::string lattice_refusal(int form, LatticeRule rule, int D, int64_t slabs, int64_t rows, int64_t cols, int periodic)
{
    const FormRow& r = kFormRows[form];
    const std::string name = std::string(r.name) + ": ";
    if (rule == LATTICE_MASK)
        return name + "periodic = " + std::to_string(periodic) + ": " + r.mask_rule;
    const std::string shape = name + lattice_shape(form, D, slabs, rows, cols) + ": ";
    if (rule == LATTICE_EXTENT)
        return shape + r.extent_rule;
    return shape + (r.axes == 3 ? "slabs*" : "") + "rows*cols" + (r.times_D ? "*D" : "") + " overflows";
}

}  // namespace lbfgsx
