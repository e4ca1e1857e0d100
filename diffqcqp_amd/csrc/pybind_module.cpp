// pybind_module.cpp -- the pybind11 face of the C ABI (include/diffqcqp_hip.h), module `diffqcqp_amd._dqq`.
//
// The reference reaches its solver through a pybind11 module (`diffqcqp`, pybindings.cpp:74-83: one call per
// PROBLEM, numpy in / numpy out).  This module is the batched counterpart: one call per BATCH, every function of
// the C ABI under its own name with the same argument order.  Pointers are passed as Python ints (what
// `torch.Tensor.data_ptr()` and `torch.cuda.current_stream().cuda_stream` return) or None; nothing is copied, no torch
// type crosses the boundary.  It adds no logic of its own -- `diffqcqp_amd/_capi.py` binds the very same symbols with
// ctypes when this module has not been built; the pybind11 call costs about a microsecond where the 16-argument
// ctypes call costs several (it matters at B = 1: the reference's published figure is a single problem).
// Host-only translation unit (g++): the HIP code is behind the C ABI.
#include <pybind11/pybind11.h>

#include <cstdint>

#include "diffqcqp_hip.h"

namespace py = pybind11;

namespace {

template <typename T>
T* ptr(const py::object& o)
{
    return o.is_none() ? nullptr : reinterpret_cast<T*>(o.cast<std::uintptr_t>());
}
using O = const py::object&;

// How a C parameter looks from Python: a pointer (T*, const T*, void*) is an int or None, every number is itself.
template <typename T>
struct Arg {
    using py_type = T;
    static T to_c(T v) { return v; }
};
template <typename T>
struct Arg<T*> {
    using py_type = O;
    static T* to_c(O o) { return ptr<T>(o); }
};

// m.def(name, ...) for a function of the C ABI without out-parameters: the lambda is derived from the function's own type,
// so the header's argument order is the module's and a changed signature cannot be bound with the old one.
template <typename R, typename... A>
void bind(py::module_& m, const char* name, R (*fn)(A...))
{
    m.def(name, [fn](typename Arg<A>::py_type... a) { return fn(Arg<A>::to_c(a)...); });
}

} // namespace

PYBIND11_MODULE(_dqq, m)
{
    m.doc() = "pybind11 binding of libdiffqcqp_hip.so (include/diffqcqp_hip.h): batched ADMM QP / QCQP on MI355X";
    bind(m, "dqq_workspace_bytes", &dqq_workspace_bytes);
    bind(m, "dqq_scratch_bytes", &dqq_scratch_bytes);
    bind(m, "dqq_max_n", &dqq_max_n);
    bind(m, "dqq_workspace_reset", &dqq_workspace_reset);
    bind(m, "dqq_hint_flags", &dqq_hint_flags);
    bind(m, "dqq_qp_fwd_f64", &dqq_qp_fwd_f64);
    bind(m, "dqq_qp_bwd_f64", &dqq_qp_bwd_f64);
    bind(m, "dqq_qcqp_fwd_f64", &dqq_qcqp_fwd_f64);
    bind(m, "dqq_qcqp_bwd_f64", &dqq_qcqp_bwd_f64);
    bind(m, "dqq_boxqp_fwd_f64", &dqq_boxqp_fwd_f64);
    bind(m, "dqq_boxqp_bwd_f64", &dqq_boxqp_bwd_f64);
    bind(m, "dqq_signedboxqp_fwd_f64", &dqq_signedboxqp_fwd_f64);
    bind(m, "dqq_signedboxqp_bwd_f64", &dqq_signedboxqp_bwd_f64);
    bind(m, "dqq_fwd_warm_f64", &dqq_fwd_warm_f64);
    bind(m, "dqq_check_f64", &dqq_check_f64);
    bind(m, "dqq_equilibrate_f64", &dqq_equilibrate_f64);
    bind(m, "dqq_unscale_f64", &dqq_unscale_f64);
    bind(m, "dqq_jvp_f64", &dqq_jvp_f64);
    bind(m, "dqq_polish_scratch_bytes", &dqq_polish_scratch_bytes);
    bind(m, "dqq_polish_f64", &dqq_polish_f64);
    bind(m, "dqq_newton_scratch_bytes", &dqq_newton_scratch_bytes);
    bind(m, "dqq_newton_bwd_f64", &dqq_newton_bwd_f64);
    bind(m, "dqq_newton_jvp_f64", &dqq_newton_jvp_f64);
    bind(m, "dqq_newton_jac_scratch_bytes", &dqq_newton_jac_scratch_bytes);
    bind(m, "dqq_newton_jac_f64", &dqq_newton_jac_f64);
    bind(m, "dqq_newton_active_f64", &dqq_newton_active_f64);
    bind(m, "dqq_polish_reg_f64", &dqq_polish_reg_f64);
    bind(m, "dqq_polish_ls_f64", &dqq_polish_ls_f64);
    bind(m, "dqq_newton_bwd_reg_f64", &dqq_newton_bwd_reg_f64);
    bind(m, "dqq_newton_jvp_reg_f64", &dqq_newton_jvp_reg_f64);
    bind(m, "dqq_newton_jac_reg_f64", &dqq_newton_jac_reg_f64);
    bind(m, "dqq_polish_smooth_f64", &dqq_polish_smooth_f64);
    bind(m, "dqq_newton_bwd_smooth_f64", &dqq_newton_bwd_smooth_f64);
    bind(m, "dqq_newton_jvp_smooth_f64", &dqq_newton_jvp_smooth_f64);
    bind(m, "dqq_newton_jac_smooth_f64", &dqq_newton_jac_smooth_f64);
    bind(m, "dqq_polish_path_f64", &dqq_polish_path_f64);   // (kappas, stage_steps: addresses of HOST arrays)
    // the five with an out-parameter or bytes: written out
    m.def("dqq_workspace_status", [](O ws, std::size_t ws_bytes, O stream) {
        int dirty = 0;
        const int rc = dqq_workspace_status(ptr<const void>(ws), ws_bytes, ptr<void>(stream), &dirty);
        return py::make_tuple(rc, dirty);
    });
    m.def("dqq_device_pointer", [](O pinned_host) {
        void* dev = nullptr;
        const int rc = dqq_device_pointer(ptr<void>(pinned_host), &dev);
        return py::make_tuple(rc, reinterpret_cast<std::uintptr_t>(dev));
    });
    m.def("dqq_get_option", [](const py::bytes& name) {
        int v = 0;
        const int rc = dqq_get_option(std::string(name).c_str(), &v);
        return py::make_tuple(rc, v);
    });
    m.def("dqq_set_option", [](const py::bytes& name, int value) { return dqq_set_option(std::string(name).c_str(), value); });
    m.def("dqq_version", []() { return py::bytes(dqq_version()); });
    m.attr("DQQ_F_INFINITE_BOUNDS") = DQQ_F_INFINITE_BOUNDS;   // the per-call flag of the Newton family's box kinds
}
