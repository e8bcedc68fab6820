// lbfgspp_amd/csrc/jit_objective.hip -- term objectives compiled at run time (include/lbfgsx.h, "term objectives").
//
// The caller's text for one term is wrapped into an objective struct with the three members the kernel templates of
// lbfgs_kernels.cuh / lbfgsb_kernels.cuh ask of an OBJ (pack, tail, finish); the generated translation unit includes those
// two headers as they ship next to this library and explicitly instantiates k_eval, k_trial, k_b_eval and
// k_b_dg_maxstep_trial for it.  hipRTC compiles it for gfx950 with the floating-point contract of the build
// (-O3 -ffp-contract=off), which is what makes a re-statement of a built-in objective bit-identical to the built-in: the
// same kernel text, the same flags, the same sums.  The code object is loaded per device with hipModuleLoadData and the
// kernels are launched with hipModuleLaunchKernel from the arguments launch_args.hpp works out for both forms.
//
// Fourteen forms of objective share all of this (include/lbfgsx.h, LBFGSX_FORM_*).  A handle carries its form; the slots of the
// loaded-kernel table and everything that launches them are the same.  What the forms differ in is one row each of two tables:
// kFormRows (form_table.hpp) has what the host says about a form -- its names, what it is bound with, the rules of a shape and
// a mask -- and is shared with liblbfgsx_solver.so; kForms below has what the generator needs -- kernel names, struct members,
// the bodies' signatures, the K and D accepted, the cache key.  The generator, the validation and the refusals are written once
// and read them.
#include <dlfcn.h>
#include <hip/hiprtc.h>

#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "form_table.hpp"
#include "launch_args.hpp"

namespace {

using lbfgsx::kFormRows;

// ---- the forms: everything that differs between them in the generated translation unit, in the refusals and in the cache key
// one body of a form: the method generated around the caller's text
struct BodyDesc
{
    const char* comment;    // the comment above the method
    const char* signature;  // the method, without its qualifiers
    const char* line;       // its #line name: the compile log counts lines per body
    const char* noun;       // what messages call it
    const char* absent;     // an optional body: the method's text when the caller gives none; null: the body is required
    const char* flag;       // an optional body: the struct's constant that says whether the caller gave one
};
// what the generator needs of a form; its names in messages and entry points are its row of kFormRows (form_table.hpp)
struct FormDesc
{
    const char* obj;                          // the generated struct
    const char* includes;                     // the kernel headers
    const char* kernels[lbfgsx::JIT_NSLOTS];  // by slot; null: the form has no kernel there
    const char* members;                      // the struct's members after TermArgs' (launch_args.hpp: the form's *Args)
    BodyDesc second, body;                    // the optional body (no signature: the form has none), then the required one
    const char* rest;                         // the struct's text after the two methods
    int k_lo, k_hi, d_lo, d_hi;               // the K and D accepted
    const char *k_refusal, *d_refusal;        // '#' stands for the value refused; null: the entry point fixes the value
    bool key_second, key_d;                   // do the second body and D enter the cache key
    BodyDesc third;                          // a form of three bodies: the required one between the two (no signature: none)
};
#define TERM_SIGNATURE "T term(const T (&x)[K], T (&g)[K], int64_t i) const"
#define POINT_SIGNATURE(name) "T " name "(const T (&x)[1], T (&g)[1], int64_t i) const"
#define POINT_ABSENT "        g[0] = T(0);\n        return T(0);\n"
// the members of both linear-model forms (launch_args.hpp: LinearArgs)
#define LINEAR_MEMBERS                                                                             \
    "    const int32_t* rowptr;\n    const int32_t* col;\n    const T* val;\n"                      \
    "    const uint32_t* colptr;\n    const int32_t* trow;\n    const T* tval;\n"                   \
    "    T* w;\n    T* v;\n"                                                                       \
    "    const T* part;\n    const int32_t* long_col;\n    const uint32_t* long_chunk;\n"           \
    "    int64_t R, nnz;\n    int32_t L, C, nlong, pad_;\n"
const BodyDesc kNoBody = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
const FormDesc kForms[14] = {
    {"ObjTerm", "#include \"lbfgs_kernels.cuh\"\n#include \"lbfgsb_kernels.cuh\"\n",
     {"k_eval", "k_trial", "k_b_eval", "k_b_dg_maxstep_trial", nullptr, nullptr, "k_trial_post"}, "", kNoBody,
     {"    // one term: x[0..K) in, g[0..K) out, the term's value returned\n", TERM_SIGNATURE, "objective_body", "body", nullptr,
      nullptr},
     "    // the W / K terms of one 16-byte pack (W is a multiple of K: a term never straddles a pack)\n"
     "    template <class A>\n"
     "    __device__ __forceinline__ void pack(int64_t vi, const Pack<T>& x, Pack<T>& g, A& fx) const\n    {\n"
     "        constexpr int W = Vec16<T>::W;\n"
     "#pragma unroll\n"
     "        for (int k = 0; k < W; k += K)\n        {\n"
     "            T tx[K], tg[K];\n"
     "#pragma unroll\n"
     "            for (int j = 0; j < K; j++)\n                tx[j] = x.e[k + j];\n"
     "            const T v = term(tx, tg, vi * W + k);\n"
     "#pragma unroll\n"
     "            for (int j = 0; j < K; j++)\n                g.e[k + j] = tg[j];\n"
     "            fx.add(v);\n"
     "        }\n    }\n"
     "    __device__ __forceinline__ T finish(T sum) const { return sum; }\n"
     "    // the coordinates past the last whole pack, called for every i of them: the term that starts at i, if one does\n"
     "    template <class A>\n"
     "    __device__ __forceinline__ void tail(int64_t i, int64_t n, const T* x, T* g, A& fx) const\n    {\n"
     "        if (i % K == 0 && i + K <= n)\n        {\n"
     "            T tx[K], tg[K];\n"
     "            for (int j = 0; j < K; j++)\n                tx[j] = x[i + j];\n"
     "            const T v = term(tx, tg, i);\n"
     "            for (int j = 0; j < K; j++)\n                g[i + j] = tg[j];\n"
     "            fx.add(v);\n"
     "        }\n    }\n",
     1, 2, 1, 1,
     "K = # is not supported: a term reads K = 1 or K = 2 consecutive coordinates (a 16-byte pack of two doubles must hold whole "
     "terms)",
     nullptr, false, false},
    {"ObjChain", "#include \"chain_kernels.cuh\"\n",
     {"k_chain_eval", "k_chain_trial", "k_chain_b_eval", "k_chain_b_dg_maxstep_trial"}, "", kNoBody,
     {"    // the term that starts at coordinate i: x[0..K) in, its K partial derivatives g[0..K) out, its value returned\n",
      TERM_SIGNATURE, "objective_body", "body", nullptr, nullptr},
     "", 2, 3, 1, 1,
     "K = # is not supported: a chain term reads K = 2 or K = 3 consecutive coordinates (its halo of K - 1 values must lie inside "
     "the neighbouring 16-byte pack of two doubles)",
     nullptr, false, false},
    {"ObjGrid", "#include \"grid_kernels.cuh\"\n",
     {"k_grid_eval", "k_grid_trial", "k_grid_b_eval", "k_grid_b_dg_maxstep_trial"}, "    int64_t rows, cols;\n", kNoBody,
     {"    // the cell whose origin is node (row, col), flat index i = row*cols + col: x = {x[row,col], x[row,col+1], x[row+1,col],\n"
      "    // x[row+1,col+1]} in, its four partial derivatives g out, its value returned\n",
      "T term(const T (&x)[4], T (&g)[4], int64_t i, int64_t row, int64_t col) const", "objective_body", "body", nullptr, nullptr},
     "", 4, 4, 1, 1, "a cell reads K = 4 coordinates", nullptr, false, false},
    {"ObjGraph", "#include \"graph_kernels.cuh\"\n",
     {"k_graph_eval", "k_graph_trial", "k_graph_b_eval", "k_graph_b_dg_maxstep_trial"},
     "    const uint32_t* off;\n    const GraphEntry* inc;\n    int64_t E;\n",
     {"    // the term of node i: x[0] = x[i] in, its derivative g[0] out, its value returned\n", POINT_SIGNATURE("node"), "node_body",
      "node body", POINT_ABSENT, "kNode"},
     {"    // the term of edge e = (i, j): x = {x[i], x[j]} in, its two partial derivatives g out, its value returned\n",
      "T edge(const T (&x)[2], T (&g)[2], int64_t e, int64_t i, int64_t j) const", "edge_body", "edge body", nullptr, nullptr},
     "", 2, 2, 1, 1, "an edge reads K = 2 coordinates", nullptr, true, false},
    {"ObjMesh", "#include \"mesh_kernels.cuh\"\n",
     {"k_mesh_eval", "k_mesh_trial", "k_mesh_b_eval", "k_mesh_b_dg_maxstep_trial"},
     "    const uint32_t* off;\n    const uint32_t* inc;\n    int64_t E, N;\n",
     {"    // the term of node i: x[d] = x[i*D + d] in, its D partial derivatives g out, its value returned\n",
      "T node(const T (&x)[D], T (&g)[D], int64_t i) const", "node_body", "node body",
      "        for (int d = 0; d < D; d++)\n            g[d] = T(0);\n        return T(0);\n", "kNode"},
     {"    // the term of element e with nodes v[0..K): x[k*D + d] = unknown d of node v[k] in, its K*D partial derivatives g out,\n"
      "    // its value returned\n",
      "T elem(const T (&x)[K * D], T (&g)[K * D], int64_t e, const int64_t (&v)[K]) const", "elem_body", "element body", nullptr,
      nullptr},
     "", 2, 4, 1, 3, "K = # is not supported: an element has K = 2, 3 or 4 nodes",
     "D = # is not supported: a node has D = 1, 2 or 3 unknowns", true, true},
    {"ObjLinear", "#include \"linear_kernels.cuh\"\n",
     {"k_lin_eval", "k_lin_trial", "k_lin_b_eval", "k_lin_b_dg_maxstep_trial", "k_lin_rows", "k_lin_rows_trial"},
     LINEAR_MEMBERS,
     {"    // the term of coordinate i: x[0] = x[i] in, its derivative g[0] out, its value returned\n", POINT_SIGNATURE("coord"),
      "coord_body", "coordinate body", POINT_ABSENT, "kCoord"},
     {"    // the term of row r: z = the row's product with x in, its derivative dz out, its value returned\n",
      "T row(const T z, T& dz, int64_t r) const", "row_body", "row body", nullptr, nullptr},
     "", 1, 1, 1, 1, nullptr, nullptr, true, false},
    {"ObjLinearMulti", "#include \"linear_multi_kernels.cuh\"\n",
     {"k_linm_eval", "k_linm_trial", "k_linm_b_eval", "k_linm_b_dg_maxstep_trial", "k_linm_rows", "k_linm_rows_trial"},
     LINEAR_MEMBERS,
     {"    // the term of coordinate i = j*D + c: x[0] = x[i] in, its derivative g[0] out, its value returned\n", POINT_SIGNATURE("coord"),
      "coord_body", "coordinate body", POINT_ABSENT, "kCoord"},
     {"    // the term of row r: z[c] = the row's product with column c of the F x D matrix x in, its D partial derivatives dz out,\n"
      "    // its value returned\n",
      "T row(const T (&z)[D], T (&dz)[D], int64_t r) const", "row_body", "row body", nullptr, nullptr},
     "", 1, 1, 1, 16, nullptr, "D = # is not supported: a row has D = 1 .. 16 outputs", true, true},
    {"ObjDense", "#include \"linear_dense_kernels.cuh\"\n",
     {"k_dense_eval", "k_dense_trial", "k_dense_b_eval", "k_dense_b_dg_maxstep_trial", "k_dense_rows", "k_dense_rows_trial", nullptr,
      "k_dense_partials"},
     // launch_args.hpp: DenseArgs
     "    const T* A;\n    T* w;\n    T* v;\n    T* part;\n"
     "    int64_t R, F, lda, chunks;\n    int32_t L, C, pad0_, pad1_;\n",
     {"    // the term of coordinate i = j*D + c: x[0] = x[i] in, its derivative g[0] out, its value returned\n", POINT_SIGNATURE("coord"),
      "coord_body", "coordinate body", POINT_ABSENT, "kCoord"},
     {"    // the term of row r: z[c] = row r of the dense matrix times column c of the F x D matrix x in, its D partial derivatives\n"
      "    // dz out, its value returned\n",
      "T row(const T (&z)[D], T (&dz)[D], int64_t r) const", "row_body", "row body", nullptr, nullptr},
     "", 1, 1, 1, 16, nullptr, "D = # is not supported: a row has D = 1 .. 16 outputs", true, true},
    {"ObjLinearGraph", "#include \"linear_graph_kernels.cuh\"\n",
     {"k_ling_eval", "k_ling_trial", "k_ling_b_eval", "k_ling_b_dg_maxstep_trial", "k_lin_rows", "k_lin_rows_trial"},
     // launch_args.hpp: LinearGraphArgs
     LINEAR_MEMBERS "    const uint32_t* off;\n    const GraphEntry* inc;\n    int64_t E;\n",
     {"    // the term of coordinate i: x[0] = x[i] in, its derivative g[0] out, its value returned\n", POINT_SIGNATURE("coord"),
      "coord_body", "coordinate body", POINT_ABSENT, "kCoord"},
     {"    // the term of row r: z = the row's product with x in, its derivative dz out, its value returned\n",
      "T row(const T z, T& dz, int64_t r) const", "row_body", "row body", nullptr, nullptr},
     "", 1, 1, 1, 1, nullptr, nullptr, true, false,
     {"    // the term of edge e = (i, j): x = {x[i], x[j]} in, its two partial derivatives g out, its value returned\n",
      "T edge(const T (&x)[2], T (&g)[2], int64_t e, int64_t i, int64_t j) const", "edge_body", "edge body", nullptr, nullptr}},
    {"ObjVolume", "#include \"volume_kernels.cuh\"\n",
     {"k_volume_eval", "k_volume_trial", "k_volume_b_eval", "k_volume_b_dg_maxstep_trial"}, "    int64_t slabs, rows, cols;\n", kNoBody,
     {"    // the cell whose origin is node (slab, row, col), flat index i = (slab*rows + row)*cols + col:\n"
      "    // x[4*ds + 2*dr + dc] = x[slab+ds, row+dr, col+dc] in, its eight partial derivatives g out, its value returned\n",
      "T term(const T (&x)[8], T (&g)[8], int64_t i, int64_t slab, int64_t row, int64_t col) const", "objective_body", "body",
      nullptr, nullptr},
     "", 8, 8, 1, 1, "a cell reads K = 8 coordinates", nullptr, false, false},
    {"ObjGridPeriodic", "#include \"periodic_grid_kernels.cuh\"\n",
     {"k_pgrid_eval", "k_pgrid_trial", "k_pgrid_b_eval", "k_pgrid_b_dg_maxstep_trial"},
     // launch_args.hpp: MaskedGridArgs
     "    int64_t rows, cols;\n    int periodic, pad_;\n", kNoBody,
     {"    // the cell whose origin is node (row, col), flat index i = row*cols + col: x = {x[row,col], x[row,col+1], x[row+1,col],\n"
      "    // x[row+1,col+1]} in, + modulo the extent; j: the flat indices of those four nodes, j[0] == i; periodic: bit 0 the\n"
      "    // column direction, bit 1 the row direction; its four partial derivatives g out, its value returned\n",
      "T term(const T (&x)[4], T (&g)[4], int64_t i, int64_t row, int64_t col, const int64_t (&j)[4]) const", "objective_body",
      "body", nullptr, nullptr},
     "", 4, 4, 1, 1, "a cell reads K = 4 coordinates", nullptr, false, false},
    {"ObjVolumePeriodic", "#include \"periodic_volume_kernels.cuh\"\n",
     {"k_pvolume_eval", "k_pvolume_trial", "k_pvolume_b_eval", "k_pvolume_b_dg_maxstep_trial"},
     // launch_args.hpp: MaskedVolumeArgs
     "    int64_t slabs, rows, cols;\n    int periodic, pad_;\n", kNoBody,
     {"    // the cell whose origin is node (slab, row, col), flat index i = (slab*rows + row)*cols + col:\n"
      "    // x[4*ds + 2*dr + dc] = x[slab+ds, row+dr, col+dc] in, + modulo the extent; j: the flat indices of those eight nodes,\n"
      "    // j[0] == i; periodic: bit 0 the column, bit 1 the row, bit 2 the slab direction; its eight partial derivatives g out,\n"
      "    // its value returned\n",
      "T term(const T (&x)[8], T (&g)[8], int64_t i, int64_t slab, int64_t row, int64_t col, const int64_t (&j)[8]) const",
      "objective_body", "body", nullptr, nullptr},
     "", 8, 8, 1, 1, "a cell reads K = 8 coordinates", nullptr, false, false},
    {"ObjGridField", "#include \"grid_field_kernels.cuh\"\n",
     {"k_gfield_eval", "k_gfield_trial", "k_gfield_b_eval", "k_gfield_b_dg_maxstep_trial"},
     // launch_args.hpp: MaskedGridArgs (D is a constant of the struct)
     "    int64_t rows, cols;\n    int periodic, pad_;\n", kNoBody,
     {"    // the cell whose origin is node (row, col), node index i = row*cols + col: x[k*D + d] = unknown d of corner k in, the\n"
      "    // corners {(row,col), (row,col+1), (row+1,col), (row+1,col+1)}, + modulo the extent; j: the node indices of those four\n"
      "    // corners, j[0] == i, the flat coordinate of x[k*D + d] is j[k]*D + d; periodic: bit 0 the column direction, bit 1 the\n"
      "    // row direction; its 4*D partial derivatives g out, its value returned\n",
      "T term(const T (&x)[4 * D], T (&g)[4 * D], int64_t i, int64_t row, int64_t col, const int64_t (&j)[4]) const",
      "objective_body", "body", nullptr, nullptr},
     "", 4, 4, 1, 3, "a cell has K = 4 corners", "D = # is not supported: a node has D = 1, 2 or 3 unknowns", false, true},
    {"ObjGridStencil", "#include \"grid_stencil_kernels.cuh\"\n",
     {"k_stencil_eval", "k_stencil_trial", "k_stencil_b_eval", "k_stencil_b_dg_maxstep_trial"},
     // launch_args.hpp: MaskedGridArgs
     "    int64_t rows, cols;\n    int periodic, pad_;\n", kNoBody,
     {"    // the patch whose origin is node (row, col), flat index i = row*cols + col: x[3*dr + dc] = x[row+dr, col+dc] in, dr, dc =\n"
      "    // 0, 1, 2, + modulo the extent; j: the flat indices of those nine nodes, j[0] == i; periodic: bit 0 the column direction,\n"
      "    // bit 1 the row direction; its nine partial derivatives g out, its value returned\n",
      "T term(const T (&x)[9], T (&g)[9], int64_t i, int64_t row, int64_t col, const int64_t (&j)[9]) const", "objective_body",
      "body", nullptr, nullptr},
     "", 9, 9, 1, 1, "a patch reads K = 9 coordinates", nullptr, false, false}};
#undef LINEAR_MEMBERS
#undef TERM_SIGNATURE
#undef POINT_SIGNATURE
#undef POINT_ABSENT
// the kernels' parameter lists by slot, OBJ for the generated struct; the order the explicit instantiations are written in
const char* const kKernelParams[lbfgsx::JIT_NSLOTS] = {
    "const S*, S*, int64_t, OBJ, RedWs, S*",
    "const S*, const S*, S, S*, S*, int64_t, OBJ, RedWs, S*, int",
    "const S*, S*, const S*, const S*, int64_t, OBJ, RedWs, S*",
    "const S*, const S*, const S*, const S*, const S*, S, S*, S*, int64_t, OBJ, RedWs, S*, int",
    "const S*, OBJ",
    "const S*, const S*, S, OBJ",
    "const S*, const S*, S, S*, S*, int64_t, OBJ, RedWs, S*, int, TrialPost<S>",
    "OBJ"};
const int kEmitOrder[lbfgsx::JIT_NSLOTS] = {0, 1, 6, 2, 3, 4, 5, 7};
// does a form have the kernel of slot k: the four every form has, a linear-model objective's two row passes, a term
// objective's post form of k_trial, a dense linear-model objective's partial pass (a table row names exactly the slots of its
// form)
inline bool has_kernel(int form, int k) { return k >= 0 && k < lbfgsx::JIT_NSLOTS && kForms[form].kernels[k] != nullptr; }

// ---- hipRTC, loaded on first use (a process that never compiles an objective does not need it)
struct Rtc
{
    void* lib = nullptr;
    decltype(&hiprtcCreateProgram) create = nullptr;
    decltype(&hiprtcDestroyProgram) destroy = nullptr;
    decltype(&hiprtcAddNameExpression) add_name = nullptr;
    decltype(&hiprtcCompileProgram) compile = nullptr;
    decltype(&hiprtcGetProgramLogSize) log_size = nullptr;
    decltype(&hiprtcGetProgramLog) log = nullptr;
    decltype(&hiprtcGetLoweredName) lowered = nullptr;
    decltype(&hiprtcGetCodeSize) code_size = nullptr;
    decltype(&hiprtcGetCode) code = nullptr;
    std::string error;
};

const Rtc& rtc()
{
    static Rtc r;
    static std::once_flag once;
    std::call_once(once, []() {
        // the unversioned name first (whatever ROCm the process runs with), then the installation's own copy
        std::vector<std::string> names = {"libhiprtc.so"};
        if (const char* e = getenv("ROCM_PATH"))
            names.push_back(std::string(e) + "/lib/libhiprtc.so");
        names.push_back("/opt/rocm/lib/libhiprtc.so");
        names.push_back("libhiprtc.so.7");
        for (const std::string& n : names)
            if ((r.lib = dlopen(n.c_str(), RTLD_NOW | RTLD_LOCAL)))
                break;
        if (!r.lib)
        {
            r.error = "libhiprtc.so not found (the run-time compiler of ROCm)";
            return;
        }
#define RTC_SYM(member, name)                                             \
    r.member = reinterpret_cast<decltype(r.member)>(dlsym(r.lib, #name)); \
    if (!r.member)                                                        \
        r.error = "libhiprtc.so lacks " #name;
        RTC_SYM(create, hiprtcCreateProgram)
        RTC_SYM(destroy, hiprtcDestroyProgram)
        RTC_SYM(add_name, hiprtcAddNameExpression)
        RTC_SYM(compile, hiprtcCompileProgram)
        RTC_SYM(log_size, hiprtcGetProgramLogSize)
        RTC_SYM(log, hiprtcGetProgramLog)
        RTC_SYM(lowered, hiprtcGetLoweredName)
        RTC_SYM(code_size, hiprtcGetCodeSize)
        RTC_SYM(code, hiprtcGetCode)
#undef RTC_SYM
    });
    return r;
}

// the directory of lbfgs_kernels.cuh: csrc/ next to this library, or LBFGSX_KERNEL_DIR (include/lbfgsx.h) for a library
// installed apart from its kernel headers
std::string kernel_dir()
{
    if (const char* e = getenv("LBFGSX_KERNEL_DIR"))
        return e;
    Dl_info info;
    if (dladdr(reinterpret_cast<const void*>(&kernel_dir), &info) && info.dli_fname)
    {
        std::string p = info.dli_fname;
        const size_t k = p.rfind('/');
        return (k == std::string::npos ? std::string(".") : p.substr(0, k)) + "/csrc";
    }
    return "csrc";
}

// ---- the generated translation unit
// one method of the struct around the caller's text (null or empty: the form's text for an absent body)
void emit_body(std::string& s, const BodyDesc& b, const char* text)
{
    s += b.comment;
    s += std::string("    __device__ __forceinline__ ") + b.signature + "\n    {\n";
    if (text && *text)
        s += std::string("#line 1 \"") + b.line + "\"\n" + text + "\n#line 1 \"objective_wrapper\"\n";
    else
        s += b.absent;
    s += "    }\n";
}

// the struct the form's kernel header asks for (the leading members are TermArgs', launch_args.hpp), and the explicit
// instantiations of its kernels.  second: a graph, mesh or linear-model objective's optional body (null or empty: none); D: a
// mesh objective's unknowns per node, 1 for the other forms; third: the edge body of a form of three bodies
std::string generate(int form, int dtype, int K, const char* body, const char* second, int D, const char* third = nullptr)
{
    const FormDesc& f = kForms[form];
    std::string s;
    s += std::string("// generated by lbfgsx_objective_compile") + kFormRows[form].suffix + ": one " + kFormRows[form].name +
         " for the fused kernels\n";
    s += f.includes;
    s += "namespace lbfgsx {\n";
    s += std::string("typedef ") + (dtype == LBFGSX_F64 ? "double" : "float") + " term_scalar_t;\n";
    s += std::string("struct ") + f.obj + "\n{\n";
    s += "    typedef term_scalar_t T;\n";
    s += "    static constexpr int K = " + std::to_string(K) + ";\n";
    if (f.d_refusal)
        s += "    static constexpr int D = " + std::to_string(D) + ";\n";
    if (f.second.flag)
        s += std::string("    static constexpr bool ") + f.second.flag + " = " + (second && *second ? "true" : "false") + ";\n";
    s += "    const T* p0;\n    const T* p1;\n    const T* p2;\n    const T* p3;\n    T c[8];\n";
    s += f.members;
    if (f.second.signature)
        emit_body(s, f.second, second);
    if (f.third.signature)
        emit_body(s, f.third, third);
    emit_body(s, f.body, body);
    s += f.rest;
    s += "};\n";
    s += "typedef term_scalar_t S;\n";
    for (int k : kEmitOrder)
        if (f.kernels[k])
        {
            std::string params = kKernelParams[k];
            params.replace(params.find("OBJ"), 3, f.obj);
            s += std::string("template __global__ void ") + f.kernels[k] + "<S, " + f.obj + ">(" + params + ");\n";
        }
    s += "}  // namespace lbfgsx\n";
    return s;
}

// a refusal sentence of the table with the refused value in place of its '#'
std::string refusal(const char* rule, int value)
{
    std::string s = rule;
    const size_t k = s.find('#');
    return k == std::string::npos ? s : s.replace(k, 1, std::to_string(value));
}

bool valid_request(int form, int dtype, int K, const char* body, const char* second, int D, std::string& why,
                   const char* third = nullptr)
{
    const FormDesc& f = kForms[form];
    const std::string name = std::string(kFormRows[form].name) + ": ";
    const char* const no_asm = " contains 'asm': a term is plain C++ arithmetic, inline assembly is not accepted";
    if (dtype != LBFGSX_F64 && dtype != LBFGSX_F32)
        why = name + "unknown dtype";
    else if (f.k_refusal && (K < f.k_lo || K > f.k_hi))
        why = name + refusal(f.k_refusal, K);
    else if (f.d_refusal && (D < f.d_lo || D > f.d_hi))
        why = name + refusal(f.d_refusal, D);
    else if (f.third.signature && (!third || !*third))
        why = name + "empty " + f.third.noun;
    else if (!body || !*body)
        why = name + "empty " + f.body.noun;
    else if (f.third.signature && std::strstr(third, "asm"))
        why = name + "the " + f.third.noun + no_asm;
    else if (std::strstr(body, "asm"))
        why = name + "the " + f.body.noun + no_asm;
    else if (f.second.signature && second && std::strstr(second, "asm"))
        why = name + "the " + f.second.noun + no_asm;
    else
        return true;
    return false;
}

// ---- what the code object says about a kernel: its descriptor (symbol <name>.kd, 64 bytes: private segment size at
// byte 4, compute_pgm_rsrc1 at byte 48) and, where the symbol table has them, the assembler's <name>.num_vgpr /
// <name>.num_agpr absolute symbols
struct Elf64Ehdr
{
    unsigned char ident[16];
    uint16_t type, machine;
    uint32_t version;
    uint64_t entry, phoff, shoff;
    uint32_t flags;
    uint16_t ehsize, phentsize, phnum, shentsize, shnum, shstrndx;
};
struct Elf64Shdr
{
    uint32_t name, type;
    uint64_t flags, addr, offset, size;
    uint32_t link, info;
    uint64_t addralign, entsize;
};
struct Elf64Sym
{
    uint32_t name;
    unsigned char info, other;
    uint16_t shndx;
    uint64_t value, size;
};

bool find_symbol(const std::vector<char>& co, const std::string& name, Elf64Sym& out)
{
    if (co.size() < sizeof(Elf64Ehdr) || std::memcmp(co.data(), "\177ELF", 4) != 0)
        return false;
    Elf64Ehdr eh;
    std::memcpy(&eh, co.data(), sizeof(eh));
    if (eh.shentsize != sizeof(Elf64Shdr) || eh.shoff + uint64_t(eh.shnum) * sizeof(Elf64Shdr) > co.size())
        return false;
    std::vector<Elf64Shdr> sh(eh.shnum);
    std::memcpy(sh.data(), co.data() + eh.shoff, sh.size() * sizeof(Elf64Shdr));
    for (const Elf64Shdr& t : sh)
    {
        if ((t.type != 2 && t.type != 11) || t.link >= sh.size() || t.offset + t.size > co.size())  // SHT_SYMTAB, SHT_DYNSYM
            continue;
        const Elf64Shdr& str = sh[t.link];
        if (str.offset + str.size > co.size())
            continue;
        for (uint64_t k = 0; k + sizeof(Elf64Sym) <= t.size; k += sizeof(Elf64Sym))
        {
            Elf64Sym sy;
            std::memcpy(&sy, co.data() + t.offset + k, sizeof(sy));
            if (sy.name >= str.size)
                continue;
            const char* nm = co.data() + str.offset + sy.name;
            const size_t room = size_t(str.size - sy.name);
            if (name.size() < room && std::memcmp(nm, name.c_str(), name.size() + 1) == 0)
            {
                out = sy;
                return true;
            }
        }
    }
    return false;
}

bool kernel_resources(const std::vector<char>& co, const std::string& kernel, long long& vgprs, long long& scratch)
{
    Elf64Sym kd;
    if (!find_symbol(co, kernel + ".kd", kd))
        return false;
    Elf64Ehdr eh;
    std::memcpy(&eh, co.data(), sizeof(eh));
    uint64_t off = 0;
    bool found = false;
    for (int k = 0; k < eh.shnum && !found; k++)
    {
        Elf64Shdr t;
        std::memcpy(&t, co.data() + eh.shoff + uint64_t(k) * sizeof(Elf64Shdr), sizeof(t));
        if (t.type != 8 && t.addr <= kd.value && kd.value + 64 <= t.addr + t.size)  // not SHT_NOBITS
        {
            off = t.offset + (kd.value - t.addr);
            found = true;
        }
    }
    if (!found || off + 64 > co.size())
        return false;
    uint32_t priv = 0, rsrc1 = 0;
    std::memcpy(&priv, co.data() + off + 4, 4);
    std::memcpy(&rsrc1, co.data() + off + 48, 4);
    scratch = priv;
    Elf64Sym nv, na;
    if (find_symbol(co, kernel + ".num_vgpr", nv))
        vgprs = (long long) nv.value + (find_symbol(co, kernel + ".num_agpr", na) ? (long long) na.value : 0);
    else
        vgprs = ((rsrc1 & 63u) + 1) * 8;  // the allocation granule of the unified register file
    return true;
}

}  // namespace

struct lbfgsx_objective
{
    struct lbfgsx_objective_code* code = nullptr;
    bool cache_hit = false;
};

// one compiled (form, body, K, D, dtype): lives until the process ends (the cache)
struct lbfgsx_objective_code
{
    lbfgsx_objective self;  // what a context's binding points to: it outlives every handle given to a caller
    int form = LBFGSX_FORM_TERM, dtype = LBFGSX_F64, K = 1, D = 1;
    std::vector<char> code;
    std::string lowered[lbfgsx::JIT_NSLOTS];
    long long vgprs[lbfgsx::JIT_NSLOTS] = {0, 0, 0, 0, 0, 0, 0, 0}, scratch[lbfgsx::JIT_NSLOTS] = {0, 0, 0, 0, 0, 0, 0, 0};
    double compile_ms = 0.0;
    struct Loaded
    {
        hipModule_t mod = nullptr;
        hipFunction_t fn[lbfgsx::JIT_NSLOTS] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    };
    std::mutex mu;
    std::map<int, Loaded> loaded;  // per device
};

namespace {

std::mutex g_cache_mu;
std::map<std::string, std::unique_ptr<lbfgsx_objective_code> >& cache()
{
    static std::map<std::string, std::unique_ptr<lbfgsx_objective_code> > m;
    return m;
}

int compile_code(int form, int dtype, int K, int D, const char* body, const char* node, const char* third,
                 std::unique_ptr<lbfgsx_objective_code>& out, std::string& log)
{
    const Rtc& r = rtc();
    if (!r.error.empty())
    {
        log = r.error;
        return LBFGSX_E_RUNTIME;
    }
    const std::string src = generate(form, dtype, K, body, node, D, third);
    // the kernel headers ask for <hip/hip_runtime.h>; hipRTC has the runtime's declarations built in, so the name resolves
    // to an empty header instead of depending on where ROCm's headers are installed
    const char* hsrc[] = {"\n"};
    const char* hname[] = {"hip/hip_runtime.h"};
    hiprtcProgram prog = nullptr;
    if (r.create(&prog, src.c_str(), "objective_wrapper", 1, hsrc, hname) != HIPRTC_SUCCESS)
    {
        log = "hiprtcCreateProgram failed";
        return LBFGSX_E_RUNTIME;
    }
    std::string expr[lbfgsx::JIT_NSLOTS];
    const int nk = lbfgsx::JIT_NSLOTS;
    for (int k = 0; k < nk; k++)
    {
        if (!has_kernel(form, k))
            continue;
        expr[k] = std::string("lbfgsx::") + kForms[form].kernels[k] + "<lbfgsx::term_scalar_t, lbfgsx::" + kForms[form].obj + ">";
        (void) r.add_name(prog, expr[k].c_str());
    }
    const std::string inc = "-I" + kernel_dir();
    const char* opts[] = {"--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", inc.c_str()};
    const auto t0 = std::chrono::steady_clock::now();
    const hiprtcResult res = r.compile(prog, int(sizeof(opts) / sizeof(opts[0])), opts);
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    size_t ls = 0;
    if (r.log_size(prog, &ls) == HIPRTC_SUCCESS && ls > 1)
    {
        log.assign(ls, '\0');
        (void) r.log(prog, &log[0]);
        while (!log.empty() && log.back() == '\0')
            log.pop_back();
    }
    if (res != HIPRTC_SUCCESS)
    {
        if (log.empty())
            log = "hipRTC could not compile the objective";
        (void) r.destroy(&prog);
        return LBFGSX_E_INVALID;
    }
    std::unique_ptr<lbfgsx_objective_code> code(new lbfgsx_objective_code());
    code->form = form;
    code->dtype = dtype;
    code->K = K;
    code->D = D;
    code->compile_ms = ms;
    size_t cs = 0;
    bool ok = r.code_size(prog, &cs) == HIPRTC_SUCCESS && cs > 0;
    if (ok)
    {
        code->code.resize(cs);
        ok = r.code(prog, code->code.data()) == HIPRTC_SUCCESS;
    }
    for (int k = 0; ok && k < nk; k++)
    {
        if (!has_kernel(form, k))
            continue;
        const char* low = nullptr;
        ok = r.lowered(prog, expr[k].c_str(), &low) == HIPRTC_SUCCESS && low;
        if (ok)
        {
            code->lowered[k] = low;
            ok = kernel_resources(code->code, code->lowered[k], code->vgprs[k], code->scratch[k]);
        }
    }
    (void) r.destroy(&prog);
    if (!ok)
    {
        log = std::string(kFormRows[form].name) + ": the compiled code object lacks a kernel or its descriptor";
        return LBFGSX_E_RUNTIME;
    }
    code->self.code = code.get();
    out = std::move(code);
    return LBFGSX_OK;
}

void put_log(char* log, size_t log_len, const std::string& text)
{
    if (log && log_len > 0)
        std::snprintf(log, log_len, "%s", text.c_str());
}

}  // namespace

namespace lbfgsx {

int jit_launch(lbfgsx_ctx* c, int which, int grid, void** params)
{
    hipFunction_t fn = c->term ? static_cast<hipFunction_t>(c->term_fn[which]) : nullptr;  // resolved by lbfgsx_objective_bind
    if (!fn)
    {
        set_error("term objective: no kernel loaded for this context (lbfgsx_objective_bind)");
        return LBFGSX_E_LOGIC;
    }
    counters().launches.fetch_add(1, std::memory_order_relaxed);
    if (host_trace_on())
        host_trace(kForms[c->term->code->form].kernels[which]);
    LBFGSX_HIP(hipModuleLaunchKernel(fn, unsigned(grid), 1, 1, unsigned(kBlock), 1, 1, 0, c->stream, params, nullptr));
    return LBFGSX_OK;
}

}  // namespace lbfgsx

namespace {

long long objective_source(int form, int dtype, int K, const char* body, char* out, size_t len, const char* node = nullptr,
                           int D = 1, const char* third = nullptr)
{
    std::string why;
    if (!valid_request(form, dtype, K, body, node, D, why, third))
    {
        lbfgsx::set_error(why);
        return LBFGSX_E_INVALID;
    }
    const std::string s = generate(form, dtype, K, body, node, D, third);
    if (out && len > 0)
        std::snprintf(out, len, "%s", s.c_str());
    return (long long) s.size() + 1;
}

int objective_compile(int form, lbfgsx_objective** out, int dtype, int K, const char* body, char* log, size_t log_len,
                      const char* node = nullptr, int D = 1, const char* third = nullptr)
{
    if (log && log_len > 0)
        log[0] = '\0';
    if (!out)
        return LBFGSX_E_INVALID;
    *out = nullptr;
    std::string why;
    if (!valid_request(form, dtype, K, body, node, D, why, third))
    {
        lbfgsx::set_error(why);
        put_log(log, log_len, why);
        return LBFGSX_E_INVALID;
    }
    std::string key = std::to_string(form) + "/" + std::to_string(dtype) + "/" + std::to_string(K) + "/" + body;
    if (kForms[form].key_second)
        key += std::string("\x1f") + (node ? node : "");  // both bodies
    if (kForms[form].third.signature)
        key += std::string("\x1f") + third;  // all three
    if (kForms[form].key_d)
        key += "\x1f" + std::to_string(D);
    std::lock_guard<std::mutex> lock(g_cache_mu);
    auto it = cache().find(key);
    const bool hit = it != cache().end();
    if (!hit)
    {
        std::unique_ptr<lbfgsx_objective_code> code;
        std::string text;
        const int rc = compile_code(form, dtype, K, D, body, node, third, code, text);
        if (rc)
        {
            lbfgsx::set_error(std::string(kFormRows[form].name) + ": compilation failed\n" + text);
            put_log(log, log_len, text);
            return rc;
        }
        put_log(log, log_len, text);  // warnings
        it = cache().emplace(key, std::move(code)).first;
    }
    lbfgsx_objective* h = new lbfgsx_objective();
    h->code = it->second.get();
    h->cache_hit = hit;
    *out = h;
    return LBFGSX_OK;
}

}  // namespace

extern "C" {

long long lbfgsx_objective_source(int dtype, int K, const char* body, char* out, size_t len)
{
    return objective_source(LBFGSX_FORM_TERM, dtype, K, body, out, len);
}
long long lbfgsx_objective_source_chain(int dtype, int K, const char* body, char* out, size_t len)
{
    return objective_source(LBFGSX_FORM_CHAIN, dtype, K, body, out, len);
}
long long lbfgsx_objective_source_grid(int dtype, const char* body, char* out, size_t len)
{
    return objective_source(LBFGSX_FORM_GRID, dtype, 4, body, out, len);
}
long long lbfgsx_objective_source_volume(int dtype, const char* body, char* out, size_t len)
{
    return objective_source(LBFGSX_FORM_VOLUME, dtype, 8, body, out, len);
}
long long lbfgsx_objective_source_grid_periodic(int dtype, const char* body, char* out, size_t len)
{
    return objective_source(LBFGSX_FORM_GRID_PERIODIC, dtype, 4, body, out, len);
}
long long lbfgsx_objective_source_volume_periodic(int dtype, const char* body, char* out, size_t len)
{
    return objective_source(LBFGSX_FORM_VOLUME_PERIODIC, dtype, 8, body, out, len);
}
long long lbfgsx_objective_source_grid_field(int dtype, int D, const char* body, char* out, size_t len)
{
    return objective_source(LBFGSX_FORM_GRID_FIELD, dtype, 4, body, out, len, nullptr, D);
}
long long lbfgsx_objective_source_grid_stencil(int dtype, const char* body, char* out, size_t len)
{
    return objective_source(LBFGSX_FORM_GRID_STENCIL, dtype, 9, body, out, len);
}
long long lbfgsx_objective_source_graph(int dtype, const char* node_body, const char* edge_body, char* out, size_t len)
{
    return objective_source(LBFGSX_FORM_GRAPH, dtype, 2, edge_body, out, len, node_body);
}
long long lbfgsx_objective_source_mesh(int dtype, int K, int D, const char* node_body, const char* elem_body, char* out, size_t len)
{
    return objective_source(LBFGSX_FORM_MESH, dtype, K, elem_body, out, len, node_body, D);
}
long long lbfgsx_objective_source_linear(int dtype, const char* coord_body, const char* row_body, char* out, size_t len)
{
    return objective_source(LBFGSX_FORM_LINEAR, dtype, 1, row_body, out, len, coord_body);
}
long long lbfgsx_objective_source_linear_multi(int dtype, int D, const char* coord_body, const char* row_body, char* out,
                                               size_t len)
{
    return objective_source(LBFGSX_FORM_LINEAR_MULTI, dtype, 1, row_body, out, len, coord_body, D);
}
long long lbfgsx_objective_source_dense(int dtype, int D, const char* coord_body, const char* row_body, char* out, size_t len)
{
    return objective_source(LBFGSX_FORM_DENSE, dtype, 1, row_body, out, len, coord_body, D);
}
long long lbfgsx_objective_source_linear_graph(int dtype, const char* coord_body, const char* edge_body, const char* row_body,
                                               char* out, size_t len)
{
    return objective_source(LBFGSX_FORM_LINEAR_GRAPH, dtype, 1, row_body, out, len, coord_body, 1, edge_body);
}

int lbfgsx_objective_compile(lbfgsx_objective** out, int dtype, int K, const char* body, char* log, size_t log_len)
{
    return objective_compile(LBFGSX_FORM_TERM, out, dtype, K, body, log, log_len);
}
int lbfgsx_objective_compile_chain(lbfgsx_objective** out, int dtype, int K, const char* body, char* log, size_t log_len)
{
    return objective_compile(LBFGSX_FORM_CHAIN, out, dtype, K, body, log, log_len);
}
int lbfgsx_objective_compile_grid(lbfgsx_objective** out, int dtype, const char* body, char* log, size_t log_len)
{
    return objective_compile(LBFGSX_FORM_GRID, out, dtype, 4, body, log, log_len);
}
int lbfgsx_objective_compile_volume(lbfgsx_objective** out, int dtype, const char* body, char* log, size_t log_len)
{
    return objective_compile(LBFGSX_FORM_VOLUME, out, dtype, 8, body, log, log_len);
}
int lbfgsx_objective_compile_grid_periodic(lbfgsx_objective** out, int dtype, const char* body, char* log, size_t log_len)
{
    return objective_compile(LBFGSX_FORM_GRID_PERIODIC, out, dtype, 4, body, log, log_len);
}
int lbfgsx_objective_compile_volume_periodic(lbfgsx_objective** out, int dtype, const char* body, char* log, size_t log_len)
{
    return objective_compile(LBFGSX_FORM_VOLUME_PERIODIC, out, dtype, 8, body, log, log_len);
}
int lbfgsx_objective_compile_grid_field(lbfgsx_objective** out, int dtype, int D, const char* body, char* log, size_t log_len)
{
    return objective_compile(LBFGSX_FORM_GRID_FIELD, out, dtype, 4, body, log, log_len, nullptr, D);
}
int lbfgsx_objective_compile_grid_stencil(lbfgsx_objective** out, int dtype, const char* body, char* log, size_t log_len)
{
    return objective_compile(LBFGSX_FORM_GRID_STENCIL, out, dtype, 9, body, log, log_len);
}
int lbfgsx_objective_compile_graph(lbfgsx_objective** out, int dtype, const char* node_body, const char* edge_body, char* log,
                                   size_t log_len)
{
    return objective_compile(LBFGSX_FORM_GRAPH, out, dtype, 2, edge_body, log, log_len, node_body);
}
int lbfgsx_objective_compile_mesh(lbfgsx_objective** out, int dtype, int K, int D, const char* node_body, const char* elem_body,
                                  char* log, size_t log_len)
{
    return objective_compile(LBFGSX_FORM_MESH, out, dtype, K, elem_body, log, log_len, node_body, D);
}
int lbfgsx_objective_compile_linear(lbfgsx_objective** out, int dtype, const char* coord_body, const char* row_body, char* log,
                                    size_t log_len)
{
    return objective_compile(LBFGSX_FORM_LINEAR, out, dtype, 1, row_body, log, log_len, coord_body);
}
int lbfgsx_objective_compile_linear_multi(lbfgsx_objective** out, int dtype, int D, const char* coord_body, const char* row_body,
                                          char* log, size_t log_len)
{
    return objective_compile(LBFGSX_FORM_LINEAR_MULTI, out, dtype, 1, row_body, log, log_len, coord_body, D);
}
int lbfgsx_objective_compile_dense(lbfgsx_objective** out, int dtype, int D, const char* coord_body, const char* row_body, char* log,
                                   size_t log_len)
{
    return objective_compile(LBFGSX_FORM_DENSE, out, dtype, 1, row_body, log, log_len, coord_body, D);
}
int lbfgsx_objective_compile_linear_graph(lbfgsx_objective** out, int dtype, const char* coord_body, const char* edge_body,
                                          const char* row_body, char* log, size_t log_len)
{
    return objective_compile(LBFGSX_FORM_LINEAR_GRAPH, out, dtype, 1, row_body, log, log_len, coord_body, 1, edge_body);
}

void lbfgsx_objective_destroy(lbfgsx_objective* obj) { delete obj; }

int lbfgsx_objective_info(const lbfgsx_objective* obj, long long out[8])
{
    if (!obj || !out)
        return LBFGSX_E_INVALID;
    const lbfgsx_objective_code* k = obj->code;
    out[0] = out[1] = 0;
    for (int j = 0; j < lbfgsx::JIT_NSLOTS; j++)  // the maxima cover the row passes and the post form of k_trial
    {
        if (!has_kernel(k->form, j))
            continue;
        out[0] = k->vgprs[j] > out[0] ? k->vgprs[j] : out[0];
        out[1] = k->scratch[j] > out[1] ? k->scratch[j] : out[1];
        if (j < lbfgsx::JIT_NKERNELS)
            out[4 + j] = k->scratch[j];
    }
    out[2] = obj->cache_hit ? 1 : 0;
    out[3] = (long long) (k->compile_ms + 0.5);
    return LBFGSX_OK;
}

int lbfgsx_objective_K(const lbfgsx_objective* obj) { return obj ? obj->code->K : LBFGSX_E_INVALID; }
int lbfgsx_objective_dim(const lbfgsx_objective* obj) { return obj ? obj->code->D : LBFGSX_E_INVALID; }
int lbfgsx_objective_D(const lbfgsx_objective* obj) { return obj ? obj->code->D : LBFGSX_E_INVALID; }
int lbfgsx_objective_dtype(const lbfgsx_objective* obj) { return obj ? obj->code->dtype : LBFGSX_E_INVALID; }
int lbfgsx_objective_form(const lbfgsx_objective* obj) { return obj ? obj->code->form : LBFGSX_E_INVALID; }

int lbfgsx_objective_upload_count(lbfgsx_ctx* c, int slot, const void* host, int64_t count, void** dev)
{
    if (!c || slot < 0 || slot >= 4 || !host)
    {
        lbfgsx::set_error("lbfgsx_objective_upload: a term objective has four data arrays, slots 0..3");
        return LBFGSX_E_INVALID;
    }
    if (count < 1)
    {
        lbfgsx::set_error("lbfgsx_objective_upload_count: count = " + std::to_string(count) + ": a data array has at least one element");
        return LBFGSX_E_INVALID;
    }
    lbfgsx::DeviceGuard dev_guard_(c->device);
    if (c->term_own[slot] && c->term_own_count[slot] != count)
    {
        LBFGSX_HIP(lbfgsx::stream_sync(c->stream));
        (void) hipFree(c->term_own[slot]);
        c->term_own[slot] = nullptr;
    }
    if (!c->term_own[slot])
    {
        LBFGSX_HIP(hipMalloc(&c->term_own[slot], size_t(count) * c->esz));
        c->term_own_count[slot] = count;
    }
    LBFGSX_HIP(lbfgsx::copy_async(c->term_own[slot], host, size_t(count) * c->esz, hipMemcpyHostToDevice, c->stream));
    LBFGSX_HIP(lbfgsx::stream_sync(c->stream));
    if (dev)
        *dev = c->term_own[slot];
    return LBFGSX_OK;
}

int lbfgsx_objective_upload(lbfgsx_ctx* c, int slot, const void* host, void** dev)
{
    return lbfgsx_objective_upload_count(c, slot, host, c ? c->n : 0, dev);
}

}  // extern "C"

namespace {

// lbfgsx_objective_bind, lbfgsx_objective_bind_grid and lbfgsx_objective_bind_volume: rows = cols = 0 for a handle without a
// shape, slabs = 0 for every form but a volume objective, periodic = 0 for every form but the two periodic ones
int objective_bind(lbfgsx_ctx* c, const lbfgsx_objective* obj, int64_t rows, int64_t cols, const void* const p[4],
                   const double cs[8], int* id, int64_t slabs = 0, int periodic = 0)
{
    c->st_valid = false;
    c->spec_valid = false;
    if (!obj)
    {
        c->term = nullptr;
        c->term_np = 0;
        c->term_form = LBFGSX_FORM_TERM;
        c->term_slabs = c->term_rows = c->term_cols = 0;
        c->term_periodic = 0;
        if (c->graph_inc || c->lin.colptr || c->dense.w)
        {
            lbfgsx::DeviceGuard dev_guard_(c->device);
            (void) lbfgsx::stream_sync(c->stream);  // no launch still walks the list
            lbfgsx::graph_topology_free(c);
        }
        if (id)
            *id = LBFGSX_OBJ_NONE;
        return LBFGSX_OK;
    }
    lbfgsx_objective_code* code = obj->code;
    if (code->dtype != c->dtype)
    {
        lbfgsx::set_error("lbfgsx_objective_bind: the objective was compiled for the other dtype");
        return LBFGSX_E_INVALID;
    }
    if (code->form == LBFGSX_FORM_CHAIN)
    {
        if (c->n < code->K)
        {
            lbfgsx::set_error("chain objective: n = " + std::to_string(c->n) + " is less than K = " + std::to_string(code->K) +
                              ": there is no term");
            return LBFGSX_E_INVALID;
        }
    }
    else if (code->form == LBFGSX_FORM_MESH && c->n % code->D != 0)
    {
        lbfgsx::set_error("mesh objective: n = " + std::to_string(c->n) + " is not a multiple of D = " + std::to_string(code->D) +
                          ": x holds D unknowns per node");
        return LBFGSX_E_INVALID;
    }
    else if (code->form == LBFGSX_FORM_TERM && c->n % code->K != 0)
    {
        lbfgsx::set_error("term objective: n = " + std::to_string(c->n) + " is not a multiple of K = " + std::to_string(code->K));
        return LBFGSX_E_INVALID;
    }
    lbfgsx::DeviceGuard dev_guard_(c->device);
    {
        std::lock_guard<std::mutex> lock(code->mu);
        auto it = code->loaded.find(c->device);
        if (it == code->loaded.end())
        {
            lbfgsx_objective_code::Loaded l;
            LBFGSX_HIP(hipModuleLoadData(&l.mod, code->code.data()));
            for (int k = 0; k < lbfgsx::JIT_NSLOTS; k++)
                if (has_kernel(code->form, k))
                    LBFGSX_HIP(hipModuleGetFunction(&l.fn[k], l.mod, code->lowered[k].c_str()));
            it = code->loaded.emplace(c->device, l).first;
        }
        for (int k = 0; k < lbfgsx::JIT_NSLOTS; k++)
            c->term_fn[k] = it->second.fn[k];
    }
    if (code->form != LBFGSX_FORM_GRAPH && code->form != LBFGSX_FORM_MESH && !lbfgsx::form_is_linear(code->form) &&
        code->form != LBFGSX_FORM_DENSE && code->form != LBFGSX_FORM_LINEAR_GRAPH &&
        (c->graph_inc || c->lin.colptr || c->dense.w))
    {
        (void) lbfgsx::stream_sync(c->stream);  // no launch still walks the list
        lbfgsx::graph_topology_free(c);
    }
    c->term = &code->self;
    c->term_form = code->form;
    c->term_slabs = slabs;
    c->term_rows = rows;
    c->term_cols = cols;
    c->term_periodic = periodic;
    c->term_np = 0;
    for (int j = 0; j < 4; j++)
    {
        c->term_p[j] = p ? p[j] : nullptr;
        c->term_np += c->term_p[j] ? 1 : 0;
    }
    for (int j = 0; j < 8; j++)
        c->term_c[j] = cs ? cs[j] : 0.0;
    if (id)
        *id = LBFGSX_OBJ_BOUND;
    return LBFGSX_OK;
}

// is the handle one of `form`; the refusal names lbfgsx_objective_bind<suffix>, the call that asked
bool handle_is(const lbfgsx_objective* obj, int form)
{
    const lbfgsx::FormRow& f = kFormRows[form];
    if (obj->code->form == form)
        return true;
    lbfgsx::set_error(std::string("lbfgsx_objective_bind") + f.suffix + ": the handle is a " + kFormRows[obj->code->form].name +
                      ", not a " + f.name + " (lbfgsx_objective_compile" + f.suffix + ")");
    return false;
}

// the start of a bind that builds the form's list on the context (graph, mesh, linear-model): whatever is refused, here or
// by the caller's own checks or by the build, leaves no objective bound, so nothing can be launched on refused indices
int bind_begin(lbfgsx_ctx* c, const lbfgsx_objective* obj, int form)
{
    c->st_valid = false;
    c->spec_valid = false;
    c->term = nullptr;
    c->term_np = 0;
    c->term_form = LBFGSX_FORM_TERM;
    if (!handle_is(obj, form))
        return LBFGSX_E_INVALID;
    if (obj->code->dtype != c->dtype)
    {
        lbfgsx::set_error("lbfgsx_objective_bind: the objective was compiled for the other dtype");
        return LBFGSX_E_INVALID;
    }
    return LBFGSX_OK;
}

// its end: the handle bound over the list that was built, or the list freed
int bind_end(lbfgsx_ctx* c, const lbfgsx_objective* obj, const void* const p[4], const double cs[8], int* id)
{
    const int rc = objective_bind(c, obj, 0, 0, p, cs, id);
    if (rc)
    {
        lbfgsx::DeviceGuard dev_guard_(c->device);
        lbfgsx::graph_topology_free(c);
    }
    return rc;
}

// the bind of a lattice form: the handle's form, then the rules of the form's row (form_table.hpp) -- the extents, the product
// that is n (an overflow is a product that is not), the mask --, then the handle bound with them.  slabs = 0 on two axes,
// periodic = 0 for a form without a mask
int shaped_bind(lbfgsx_ctx* c, const lbfgsx_objective* obj, int form, int64_t slabs, int64_t rows, int64_t cols, int periodic,
                const void* const p[4], const double cs[8], int* id)
{
    if (!c || !obj)
        return LBFGSX_E_INVALID;
    if (!handle_is(obj, form))
        return LBFGSX_E_INVALID;
    const int D = obj->code->D;
    long long n = 0;
    const lbfgsx::LatticeRule bad = lbfgsx::lattice_check(form, D, slabs, rows, cols, periodic, &n);
    if (bad == lbfgsx::LATTICE_OVERFLOW || (bad != lbfgsx::LATTICE_EXTENT && n != (long long) c->n))
        lbfgsx::set_error(std::string(kFormRows[form].name) + ": " + lbfgsx::lattice_shape(form, D, slabs, rows, cols) +
                          " does not multiply to n = " + std::to_string(c->n));
    else if (bad)
        lbfgsx::set_error(lbfgsx::lattice_refusal(form, bad, D, slabs, rows, cols, periodic));
    else
        return objective_bind(c, obj, rows, cols, p, cs, id, slabs, periodic);
    return LBFGSX_E_INVALID;
}

}  // namespace

extern "C" {

int lbfgsx_objective_bind(lbfgsx_ctx* c, const lbfgsx_objective* obj, const void* const p[4], const double cs[8], int* id)
{
    if (!c)
        return LBFGSX_E_INVALID;
    if (obj && kFormRows[obj->code->form].bound_with)
    {
        lbfgsx::set_error(lbfgsx::unshaped_refusal(obj->code->form, false));
        return LBFGSX_E_INVALID;
    }
    return objective_bind(c, obj, 0, 0, p, cs, id);
}

// ---- the six lattice forms: one bind (shaped_bind), by the form's row of kFormRows
int lbfgsx_objective_bind_grid(lbfgsx_ctx* c, const lbfgsx_objective* obj, int64_t rows, int64_t cols, const void* const p[4],
                               const double cs[8], int* id)
{
    return shaped_bind(c, obj, LBFGSX_FORM_GRID, 0, rows, cols, 0, p, cs, id);
}
int lbfgsx_objective_bind_volume(lbfgsx_ctx* c, const lbfgsx_objective* obj, int64_t slabs, int64_t rows, int64_t cols,
                                 const void* const p[4], const double cs[8], int* id)
{
    return shaped_bind(c, obj, LBFGSX_FORM_VOLUME, slabs, rows, cols, 0, p, cs, id);
}
int lbfgsx_objective_bind_grid_periodic(lbfgsx_ctx* c, const lbfgsx_objective* obj, int64_t rows, int64_t cols, int periodic,
                                        const void* const p[4], const double cs[8], int* id)
{
    return shaped_bind(c, obj, LBFGSX_FORM_GRID_PERIODIC, 0, rows, cols, periodic, p, cs, id);
}
int lbfgsx_objective_bind_volume_periodic(lbfgsx_ctx* c, const lbfgsx_objective* obj, int64_t slabs, int64_t rows, int64_t cols,
                                          int periodic, const void* const p[4], const double cs[8], int* id)
{
    return shaped_bind(c, obj, LBFGSX_FORM_VOLUME_PERIODIC, slabs, rows, cols, periodic, p, cs, id);
}
int lbfgsx_objective_bind_grid_field(lbfgsx_ctx* c, const lbfgsx_objective* obj, int64_t rows, int64_t cols, int periodic,
                                     const void* const p[4], const double cs[8], int* id)
{
    return shaped_bind(c, obj, LBFGSX_FORM_GRID_FIELD, 0, rows, cols, periodic, p, cs, id);
}
int lbfgsx_objective_bind_grid_stencil(lbfgsx_ctx* c, const lbfgsx_objective* obj, int64_t rows, int64_t cols, int periodic,
                                       const void* const p[4], const double cs[8], int* id)
{
    return shaped_bind(c, obj, LBFGSX_FORM_GRID_STENCIL, 0, rows, cols, periodic, p, cs, id);
}

// what was bound, read back: the forms on two axes, those on three, those with a mask
int lbfgsx_objective_shape(const lbfgsx_ctx* c, int64_t* rows, int64_t* cols)
{
    if (!c || !c->term || kFormRows[c->term_form].axes != 2)
    {
        lbfgsx::set_error("lbfgsx_objective_shape: no grid objective is bound to this context");
        return LBFGSX_E_INVALID;
    }
    if (rows)
        *rows = c->term_rows;
    if (cols)
        *cols = c->term_cols;
    return LBFGSX_OK;
}

int lbfgsx_objective_shape3(const lbfgsx_ctx* c, int64_t* slabs, int64_t* rows, int64_t* cols)
{
    if (!c || !c->term || kFormRows[c->term_form].axes != 3)
    {
        lbfgsx::set_error("lbfgsx_objective_shape3: no volume objective is bound to this context");
        return LBFGSX_E_INVALID;
    }
    if (slabs)
        *slabs = c->term_slabs;
    if (rows)
        *rows = c->term_rows;
    if (cols)
        *cols = c->term_cols;
    return LBFGSX_OK;
}

int lbfgsx_objective_periodic(const lbfgsx_ctx* c, int* mask)
{
    if (!c || !c->term || kFormRows[c->term_form].mask_hi < 0)
    {
        lbfgsx::set_error("lbfgsx_objective_periodic: no periodic grid or volume objective is bound to this context");
        return LBFGSX_E_INVALID;
    }
    if (mask)
        *mask = c->term_periodic;
    return LBFGSX_OK;
}

int lbfgsx_objective_bind_graph(lbfgsx_ctx* c, const lbfgsx_objective* obj, int64_t E, const int32_t* ei, const int32_t* ej,
                                int edges_on_device, const void* const p[4], const double cs[8], int* id)
{
    if (!c || !obj)
        return LBFGSX_E_INVALID;
    if (const int rc = bind_begin(c, obj, LBFGSX_FORM_GRAPH))
        return rc;
    const int64_t lim = 2147483647;
    if (E < 1 || !ei || !ej)
    {
        lbfgsx::set_error("graph objective: E = " + std::to_string(E) + ": a graph objective has at least one edge (E >= 1) and both index arrays");
        return LBFGSX_E_INVALID;
    }
    if (E > lim)
    {
        lbfgsx::set_error("graph objective: E = " + std::to_string(E) + " exceeds 2^31 - 1 = " + std::to_string(lim) +
                          ": an incidence entry holds (e << 1) | side in 32 bits");
        return LBFGSX_E_INVALID;
    }
    if (c->n > lim)
    {
        lbfgsx::set_error("graph objective: n = " + std::to_string(c->n) + " exceeds 2^31 - 1 = " + std::to_string(lim) +
                          ": node indices are int32");
        return LBFGSX_E_INVALID;
    }
    {
        lbfgsx::DeviceGuard dev_guard_(c->device);
        const int rc = lbfgsx::graph_topology_build(c, ei, ej, E, edges_on_device);
        if (rc)
            return rc;
    }
    return bind_end(c, obj, p, cs, id);
}

int lbfgsx_objective_topology(lbfgsx_ctx* c, int64_t* E, uint32_t* off, int32_t* other, uint32_t* edge_side)
{
    if (!c || !c->term || (c->term_form != LBFGSX_FORM_GRAPH && c->term_form != LBFGSX_FORM_LINEAR_GRAPH) || !c->graph_inc)
    {
        lbfgsx::set_error("lbfgsx_objective_topology: no graph objective is bound to this context");
        return LBFGSX_E_INVALID;
    }
    if (E)
        *E = c->graph_E;
    lbfgsx::DeviceGuard dev_guard_(c->device);
    return lbfgsx::graph_topology_read(c, off, other, edge_side);
}

int lbfgsx_objective_bind_mesh(lbfgsx_ctx* c, const lbfgsx_objective* obj, int64_t E, const int32_t* elems, int elems_on_device,
                               const void* const p[4], const double cs[8], int* id)
{
    if (!c || !obj)
        return LBFGSX_E_INVALID;
    if (const int rc = bind_begin(c, obj, LBFGSX_FORM_MESH))
        return rc;
    const int K = obj->code->K, D = obj->code->D;
    const int64_t lim = 2147483647, elim = 1073741823;
    std::string why;
    if (E < 1 || !elems)
        why = "E = " + std::to_string(E) + ": a mesh objective has at least one element (E >= 1) and its connectivity table";
    else if (E > elim)
        why = "E = " + std::to_string(E) + " exceeds 2^30 - 1 = " + std::to_string(elim) +
              ": an incidence entry holds (e << 2) | slot in 32 bits";
    else if (c->n % D != 0)
        why = "n = " + std::to_string(c->n) + " is not a multiple of D = " + std::to_string(D) + ": x holds D unknowns per node";
    else if (c->n > lim)
        why = "n = " + std::to_string(c->n) + " exceeds 2^31 - 1 = " + std::to_string(lim) + ": node indices are int32";
    if (!why.empty())
    {
        lbfgsx::set_error("mesh objective: " + why);
        return LBFGSX_E_INVALID;
    }
    {
        lbfgsx::DeviceGuard dev_guard_(c->device);
        const int rc = lbfgsx::mesh_topology_build(c, K, D, elems, E, elems_on_device);
        if (rc)
            return rc;
    }
    return bind_end(c, obj, p, cs, id);
}

int lbfgsx_objective_mesh_topology(lbfgsx_ctx* c, int64_t* E, uint32_t* off, uint32_t* words)
{
    if (!c || !c->term || c->term_form != LBFGSX_FORM_MESH || !c->graph_inc)
    {
        lbfgsx::set_error("lbfgsx_objective_mesh_topology: no mesh objective is bound to this context");
        return LBFGSX_E_INVALID;
    }
    if (E)
        *E = c->graph_E;
    lbfgsx::DeviceGuard dev_guard_(c->device);
    return lbfgsx::mesh_topology_read(c, off, words);
}

int lbfgsx_objective_bind_linear(lbfgsx_ctx* c, const lbfgsx_objective* obj, int64_t R, int64_t nnz, const int32_t* rowptr,
                                 const int32_t* col, const void* val, int matrix_on_device, int lanes, const void* const p[4],
                                 const double cs[8], int* id)
{
    if (!c || !obj)
        return LBFGSX_E_INVALID;
    // either linear form: a multi-output handle has D = its outputs per row and a matrix of F = n / D columns
    const bool multi = obj->code->form == LBFGSX_FORM_LINEAR_MULTI;
    if (const int rc = bind_begin(c, obj, multi ? LBFGSX_FORM_LINEAR_MULTI : LBFGSX_FORM_LINEAR))
        return rc;
    const int D = multi ? obj->code->D : 1;
    const std::string name = std::string(kFormRows[obj->code->form].name) + ": ";
    const int64_t lim = 2147483647;
    std::string why;
    if (R < 1 || nnz < 1 || !rowptr || !col || !val)
        why = "R = " + std::to_string(R) + ", nnz = " + std::to_string(nnz) +
              ": a linear-model objective has at least one row and one entry (R >= 1, nnz >= 1) and its three CSR arrays";
    else if (R > lim)
        why = "R = " + std::to_string(R) + " exceeds 2^31 - 1 = " + std::to_string(lim) + ": row indices are int32";
    else if (nnz > lim)
        why = "nnz = " + std::to_string(nnz) + " exceeds 2^31 - 1 = " + std::to_string(lim) + ": row offsets are int32";
    else if (c->n > lim)
        why = "n = " + std::to_string(c->n) + " exceeds 2^31 - 1 = " + std::to_string(lim) + ": column indices are int32";
    else if (lanes < 0 || lanes > 64 || (lanes & (lanes - 1)) != 0)
        why = "lanes = " + std::to_string(lanes) + ": the lanes that share a row are 0 (by the rule) or a power of two in 1..64";
    else if (c->n % D != 0)
        why = "n = " + std::to_string(c->n) + " is not a multiple of D = " + std::to_string(D) +
              ": x holds the D weights of each feature";
    if (!why.empty())
    {
        lbfgsx::set_error(name + why);
        return LBFGSX_E_INVALID;
    }
    {
        lbfgsx::DeviceGuard dev_guard_(c->device);
        const int rc = lbfgsx::linear_topology_build(c, R, nnz, rowptr, col, val, matrix_on_device, lanes, multi ? D : 0);
        if (rc)
            return rc;
    }
    return bind_end(c, obj, p, cs, id);
}

int lbfgsx_objective_linear_topology(lbfgsx_ctx* c, int64_t info[8], uint32_t* colptr, int32_t* trow, uint32_t* tpos,
                                     int32_t* long_col, uint32_t* long_chunk, uint32_t* chunk)
{
    if (!c || !c->term || !lbfgsx::form_has_csr(c->term_form) || !c->lin.colptr)
    {
        lbfgsx::set_error("lbfgsx_objective_linear_topology: no linear-model objective is bound to this context");
        return LBFGSX_E_INVALID;
    }
    if (info)
    {
        const int64_t v[8] = {c->lin.R, c->lin.nnz, c->lin.L, c->lin.C, c->lin.nlong, c->lin.nchunks, c->lin.D, 0};
        for (int k = 0; k < 8; k++)
            info[k] = v[k];
    }
    lbfgsx::DeviceGuard dev_guard_(c->device);
    return lbfgsx::linear_topology_read(c, colptr, trow, tpos, long_col, long_chunk, chunk);
}

int lbfgsx_objective_bind_linear_graph(lbfgsx_ctx* c, const lbfgsx_objective* obj, int64_t R, int64_t nnz, const int32_t* rowptr,
                                       const int32_t* col, const void* val, int matrix_on_device, int lanes, int64_t E,
                                       const int32_t* ei, const int32_t* ej, int edges_on_device, const void* const p[4],
                                       const double cs[8], int* id)
{
    if (!c || !obj)
        return LBFGSX_E_INVALID;
    if (const int rc = bind_begin(c, obj, LBFGSX_FORM_LINEAR_GRAPH))
        return rc;
    const int64_t lim = 2147483647;
    std::string why;
    if (E < 1 || !ei || !ej)
        why = "E = " + std::to_string(E) + ": a graph-regularised linear-model objective has at least one edge (E >= 1) and both index arrays";
    else if (E > lim)
        why = "E = " + std::to_string(E) + " exceeds 2^31 - 1 = " + std::to_string(lim) +
              ": an incidence entry holds (e << 1) | side in 32 bits";
    else if (R < 1 || nnz < 1 || !rowptr || !col || !val)
        why = "R = " + std::to_string(R) + ", nnz = " + std::to_string(nnz) +
              ": a linear-model objective has at least one row and one entry (R >= 1, nnz >= 1) and its three CSR arrays";
    else if (R > lim)
        why = "R = " + std::to_string(R) + " exceeds 2^31 - 1 = " + std::to_string(lim) + ": row indices are int32";
    else if (nnz > lim)
        why = "nnz = " + std::to_string(nnz) + " exceeds 2^31 - 1 = " + std::to_string(lim) + ": row offsets are int32";
    else if (c->n > lim)
        why = "n = " + std::to_string(c->n) + " exceeds 2^31 - 1 = " + std::to_string(lim) + ": column and node indices are int32";
    else if (lanes < 0 || lanes > 64 || (lanes & (lanes - 1)) != 0)
        why = "lanes = " + std::to_string(lanes) + ": the lanes that share a row are 0 (by the rule) or a power of two in 1..64";
    if (!why.empty())
    {
        lbfgsx::set_error(std::string(kFormRows[LBFGSX_FORM_LINEAR_GRAPH].name) + ": " + why);
        return LBFGSX_E_INVALID;
    }
    {
        // the edges first, then the matrix beside them: either build validates its indices before anything else and leaves the
        // context without a list when one offends
        lbfgsx::DeviceGuard dev_guard_(c->device);
        int rc = lbfgsx::graph_topology_build(c, ei, ej, E, edges_on_device);
        if (rc)
            return rc;
        rc = lbfgsx::linear_topology_build(c, R, nnz, rowptr, col, val, matrix_on_device, lanes, 0, true);
        if (rc)
        {
            lbfgsx::graph_topology_free(c);
            return rc;
        }
    }
    return bind_end(c, obj, p, cs, id);
}

int lbfgsx_objective_bind_dense(lbfgsx_ctx* c, const lbfgsx_objective* obj, int64_t R, const void* A, int64_t lda, int a_on_device,
                                int lanes, const void* const p[4], const double cs[8], int* id)
{
    if (!c || !obj)
        return LBFGSX_E_INVALID;
    if (const int rc = bind_begin(c, obj, LBFGSX_FORM_DENSE))
        return rc;
    const int D = obj->code->D;
    const int64_t lim = 2147483647, F = c->n / D;
    std::string why;
    if (R < 1)
        why = "R = " + std::to_string(R) + ": a dense linear-model objective has at least one row (R >= 1)";
    else if (!A)
        why = "A is null: a dense linear-model objective has its R x F matrix (R = " + std::to_string(R) + ")";
    else if (c->n % D != 0)
        why = "n = " + std::to_string(c->n) + " is not a multiple of D = " + std::to_string(D) +
              ": x holds the D weights of each feature";
    else if (lda < F)
        why = "lda = " + std::to_string(lda) + " is less than F = n / D = " + std::to_string(F) +
              ": a row of the matrix holds its F values first";
    else if (R > lim)
        why = "R = " + std::to_string(R) + " exceeds 2^31 - 1 = " + std::to_string(lim);
    else if (F > lim)
        why = "F = " + std::to_string(F) + " exceeds 2^31 - 1 = " + std::to_string(lim);
    else if (lanes < 0 || lanes > 64 || (lanes & (lanes - 1)) != 0)
        why = "lanes = " + std::to_string(lanes) + ": the lanes that share a row are 0 (by the rule) or a power of two in 1..64";
    if (!why.empty())
    {
        lbfgsx::set_error("dense linear-model objective: " + why);
        return LBFGSX_E_INVALID;
    }
    {
        lbfgsx::DeviceGuard dev_guard_(c->device);
        const int rc = lbfgsx::dense_topology_build(c, R, D, A, lda, a_on_device, lanes);
        if (rc)
            return rc;
    }
    return bind_end(c, obj, p, cs, id);
}

int lbfgsx_objective_dense_info(lbfgsx_ctx* c, int64_t info[8])
{
    if (!c || !c->term || c->term_form != LBFGSX_FORM_DENSE || !c->dense.w)
    {
        lbfgsx::set_error("lbfgsx_objective_dense_info: no dense linear-model objective is bound to this context");
        return LBFGSX_E_INVALID;
    }
    if (info)
    {
        const lbfgsx_ctx::DenseTopo& d = c->dense;
        const int64_t v[8] = {d.R, d.F, d.D, d.L, d.C, d.chunks, d.lda, d.own ? 1 : 0};
        for (int k = 0; k < 8; k++)
            info[k] = v[k];
    }
    return LBFGSX_OK;
}

int lbfgsx_objective_dense_read(lbfgsx_ctx* c, void* w, void* v, void* part)
{
    if (!c || !c->term || c->term_form != LBFGSX_FORM_DENSE || !c->dense.w)
    {
        lbfgsx::set_error("lbfgsx_objective_dense_read: no dense linear-model objective is bound to this context");
        return LBFGSX_E_INVALID;
    }
    lbfgsx::DeviceGuard dev_guard_(c->device);
    return lbfgsx::dense_topology_read(c, w, v, part);
}

int lbfgsx_objective_bound(const lbfgsx_ctx* c, const void* p[4])
{
    if (!c || !p || !c->term)
        return LBFGSX_E_INVALID;
    for (int j = 0; j < 4; j++)
        p[j] = c->term_p[j];
    return LBFGSX_OK;
}

}  // extern "C"
