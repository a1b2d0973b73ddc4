"""tools/kernel_coverage.py: the mangled-symbol and rocprofv3 kernel-name parsers, on inline strings (no GPU, no built library)."""
import csv
import importlib.util
import io
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("kernel_coverage", os.path.join(ROOT, "tools", "kernel_coverage.py"))
kc = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(kc)

F16S = "_ZN2cf16conv_f16s_kernelILi3ELi3ELi16ELi2ELi2ELi2ELi4ELi1ELi1ELi0ELi1EEEvNS_10ConvParamsENS_8F16sGeomEPKDF16_"


def test_parse_mangled_template_kernels():
    assert kc.parse_mangled(F16S) == ("cf::conv_f16s_kernel", (3, 3, 16, 2, 2, 2, 4, 1, 1, 0, 1))
    assert kc.parse_mangled(F16S + ".kd") == kc.parse_mangled(F16S)
    assert kc.parse_mangled("_ZN2cf19attention_cf_kernelILi64EEEvPKflS2_lS2_lPfiiifi") == ("cf::attention_cf_kernel", (64,))
    # bool and type template arguments, a negative literal, an anonymous namespace, a kernel outside any namespace
    assert kc.parse_mangled("_ZN2cf15gn_apply_kernelILb1EEEvPKfS2_S2_S2_PfPKdiiifiiiNS_7ResNormE") == ("cf::gn_apply_kernel", (True,))
    assert kc.parse_mangled("_ZN2cf18frame_boxes_kernelIhEEvPKT_Piii") == ("cf::frame_boxes_kernel", ("unsigned char",))
    assert kc.parse_mangled("_ZN2cf3fooILin2ELj7EEEvi") == ("cf::foo", (-2, 7))
    assert kc.parse_mangled("_ZN2cf12_GLOBAL__N_116conv_wino_kernelILi4ELi1EEEvNS_10ConvParamsEPK6__halfi") == \
        ("cf::(anonymous namespace)::conv_wino_kernel", (4, 1))
    assert kc.parse_mangled("_Z20norm_head_1x1_kernelILi4EEvPKfS1_fS1_S1_Pfiii") == ("norm_head_1x1_kernel", (4,))
    assert kc.parse_mangled("_ZN2cf23window_attention_kernelEPKfS1_S1_Pfiiiiiif") == ("cf::window_attention_kernel", ())
    # variables and local statics are not kernels
    assert kc.parse_mangled("_ZN2cfL12t_conv_termsE") is None
    assert kc.parse_mangled("_ZN2cfL12g_last_errorB5cxx11E") is None
    assert kc.parse_mangled("_ZZN2cf13launch_f16s_vILi3EEEivE8attr_set") is None
    assert kc.parse_mangled("hipModuleLaunchKernel") is None


def test_parse_demangled_rocprof_names():
    assert kc.parse_demangled("void cf::conv_f16s_kernel<3, 3, 16, 2, 2, 2, 4, 1, 1, 0, 1>(cf::ConvParams, cf::F16sGeom, _Float16 const*)") == \
        kc.parse_mangled(F16S)
    assert kc.parse_demangled("void cf::(anonymous namespace)::conv_wino_kernel<4, 1>(cf::ConvParams, __half const*, int)") == \
        ("cf::(anonymous namespace)::conv_wino_kernel", (4, 1))
    assert kc.parse_demangled("void cf::gn_apply_kernel<true>(float const*, cf::ResNorm)") == ("cf::gn_apply_kernel", (True,))
    assert kc.parse_demangled("void cf::frame_boxes_kernel<unsigned char>(unsigned char const*, int*, int, int, int)") == \
        ("cf::frame_boxes_kernel", ("unsigned char",))
    assert kc.parse_demangled("cf::window_attention_kernel(float const*, float const*, float const*, float*, int, int, int, int, int, int, float)") == \
        ("cf::window_attention_kernel", ())
    assert kc.parse_demangled("void at::native::elementwise_kernel<128, 4, at::native::gpu_kernel_impl<X>(Y)::{lambda(int)#1}>(int, Z)")[0] == \
        "at::native::elementwise_kernel"
    assert kc.parse_demangled(F16S + ".kd") == kc.parse_mangled(F16S)


def _csv(header, rows):
    s = io.StringIO()
    w = csv.writer(s)
    w.writerow(header)
    w.writerows(rows)
    return s.getvalue()


def test_report_counts_trace_and_stats_csv(tmp_path):
    name = "void cf::conv_f16s_kernel<3, 3, 16, 2, 2, 2, 4, 1, 1, 0, 1>(cf::ConvParams, cf::F16sGeom, _Float16 const*)"
    trace = tmp_path / "t_kernel_trace.csv"
    trace.write_text(_csv(["Kind", "Kernel_Name", "Start_Timestamp"], [["KERNEL_DISPATCH", name, 1], ["KERNEL_DISPATCH", name, 2],
                                                                       ["KERNEL_DISPATCH", F16S.replace("Li2ELi2ELi2", "Li2ELi1ELi3"), 3]]))
    stats = tmp_path / "t_kernel_stats.csv"
    stats.write_text(_csv(["Name", "Calls", "TotalDurationNs"], [['"' + name + '"', 5, 100]]))
    got = kc.launched_kernels([str(trace), str(stats)])
    assert got[("cf::conv_f16s_kernel", (3, 3, 16, 2, 2, 2, 4, 1, 1, 0, 1))] == 7
    assert got[("cf::conv_f16s_kernel", (3, 3, 16, 2, 1, 3, 4, 1, 1, 0, 1))] == 1
    built = {"cf::conv_f16s_kernel": {(3, 3, 16, 2, 2, 2, 4, 1, 1, 0, 1), (3, 3, 16, 2, 2, 2, 4, 1, 1, 0, 3)},
             "cf::other_kernel": {()}}
    out = io.StringIO()
    assert kc.report(built, got, counts=True, out=out) == (1, 3)
    text = out.getvalue()
    assert "never launched  conv_f16s_kernel<3, 3, 16, 2, 2, 2, 4, 1, 1, 0, 3>" in text
    assert "never launched  other_kernel<>" in text
    assert "launched but not in the library: cf::conv_f16s_kernel<3, 3, 16, 2, 1, 3, 4, 1, 1, 0, 1>" in text
    out = io.StringIO()
    assert kc.report(built, got, family_re="conv_f16s", out=out) == (1, 2)
