"""lda --networks, the host side (no GPU): what the tool says before the device is opened, the network options' struct and
the new symbols.  The tool runs with no visible device, as in tests/test_lda_host.py: a refusal must come before anything
asks for one, and an accepted command line must go on to ask."""
import ctypes
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "aaltoasr_amd", "lib", "bin")

PH3 = "PHONE\n3\n" + "".join("%d 3 %s\n-1 -2 %d\n0 1 2 1.0\n1 0\n2 2 2 0.5 1 0.5\n" % (i + 1, lab, i)
                             for i, lab in enumerate(("_", "__", "a")))
HEAD = "module\n{\n  name a\n  type audiofile\n}\nmodule\n{\n  name n\n  type normalization\n  sources a\n}\n"
CFG = HEAD + "module\n{\n  name lda\n  type lin_transform\n  dim 2\n  matrix 1 0 0 0 1 0\n  sources n\n}\n"
CFG_NO_MATRIX = HEAD + "module\n{\n  name lda\n  type lin_transform\n  dim 2\n  sources n\n}\n"
NEW_SYMBOLS = ["aasr_scatter_accumulate_weighted_dev", "aasr_run_lda_networks_recipe", "aasr_lda_network_default_options",
               "aasr_lda_networks_check"]


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("lda_networks_host")
    open(str(d / "m.gk"), "w").write("3 2 diagonal_cov\n0 0 1 1\n1 1 1 1\n2 2 1 1\n")
    open(str(d / "full.gk"), "w").write("3 2 full_cov\n")
    open(str(d / "m.mc"), "w").write("3\n1 0 1.0\n1 1 1.0\n1 2 1.0\n")
    open(str(d / "m.ph"), "w").write(PH3)
    open(str(d / "nosil.ph"), "w").write(PH3.replace(" __\n", " b\n"))
    open(str(d / "f.cfg"), "w").write(CFG)
    open(str(d / "nomatrix.cfg"), "w").write(CFG_NO_MATRIX)
    open(str(d / "net.rcp"), "w").write("audio=%s hmmnet=%s\n" % (d / "a.wav", d / "a.hmmnet"))
    open(str(d / "phn.rcp"), "w").write("audio=%s transcript=%s\n" % (d / "a.wav", d / "a.phn"))
    open(str(d / "lines.rcp"), "w").write("audio=%s hmmnet=%s start-line=3 end-line=5\n" % (d / "a.wav", d / "a.hmmnet"))
    return d


def run_tool(files, *extra, model=("-b", "m"), cfg="f.cfg", recipe="net.rcp", dim="2"):
    cmd = [os.path.join(BIN, "lda"), "-c", str(files / cfg), "-r", str(files / recipe), "-M", "lda", "-d", dim]
    if model:
        cmd += [model[0], str(files / model[1])]
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")   # no device, whatever the machine has
    return subprocess.run(cmd + list(extra), capture_output=True, text=True, timeout=120, env=env)


def refused(r, *words):
    assert r.returncode == 1 and r.stderr.startswith("exception: "), r.stderr
    for w in words:
        assert w in r.stderr, (w, r.stderr)
    assert "hip" not in r.stderr.lower() and "Aborted" not in r.stderr, r.stderr


def test_segmode_needs_networks(capi, files):
    refused(run_tool(files, "--segmode", "vit", model=("-p", "m.ph"), recipe="phn.rcp"), "lda: --segmode", "--networks",
            "not supported")


@pytest.mark.parametrize("extra,words", [
    (["--networks", "--segmode", "mpv"], ["lda: --segmode mpv", "--networks", "not supported"]),
    (["--networks", "--segmode", "xyz"], ["Invalid segmentation mode xyz"]),
    (["--networks", "-O"], ["lda: -O", "--networks", "not supported"]),
])
def test_refusals_with_networks(capi, files, extra, words):
    refused(run_tool(files, *extra), *words)


def test_a_line_without_hmmnet_is_the_reference_message(capi, files):
    refused(run_tool(files, "--networks", recipe="phn.rcp"), "Recipe::Info::init_hmmnet_files: hmmnet not specified in recipe.")


def test_networks_needs_a_model(capi, files):
    refused(run_tool(files, "--networks", model=("-p", "m.ph")), "--base", "--gk", "--mc")
    refused(run_tool(files, "--networks", model=None), "--base", "--gk", "--mc")
    refused(run_tool(files, "--networks", "--mc", str(files / "m.mc"), "-p", str(files / "m.ph"), model=("-g", "full.gk")),
            "lda: only diagonal Gaussians are supported")


def test_a_module_without_a_matrix_is_named(capi, files):
    refused(run_tool(files, "--networks", cfg="nomatrix.cfg"), "lda: --networks", "module lda", "no matrix")
    # the .phn mode estimates the first matrix of such a module: there it is no refusal
    r = run_tool(files, model=("-p", "m.ph"), cfg="nomatrix.cfg", recipe="phn.rcp")
    assert r.returncode == 1 and "lda:" not in r.stderr, r.stderr


def test_the_driver_checks_come_before_the_device(capi, files):
    refused(run_tool(files, "--networks", dim="1"), "lda: -d 1 but module lda has dimension 2")
    refused(run_tool(files, "--networks", "-g", str(files / "m.gk"), "--mc", str(files / "m.mc"), model=("-p", "nosil.ph")),
            "lda: no HMM __ in the model")
    refused(run_tool(files, "--networks", recipe="lines.rcp"), "start-line / end-line")


def test_minus_h_stays_refused(capi, files):
    for opt in ("-H", "--mpv", "--vit"):
        refused(run_tool(files, "--networks", opt), "lda: " + opt, "not supported")
    r = subprocess.run([os.path.join(BIN, "lda"), "--help"], capture_output=True, text=True, timeout=60)
    line = [l for l in r.stdout.splitlines() if "--networks" in l and "hmmnet=" in l]
    assert r.returncode == 0 and len(line) == 1 and "-H" in line[0], r.stdout


@pytest.mark.parametrize("extra", [[], ["--segmode", "vit", "-F", "20", "-W", "300", "-A", "0.5"],
                                   ["--segmode", "bw", "--no-silence", "-m", "10"]])
def test_an_accepted_command_line_reaches_the_device_and_fails_there(capi, files, extra):
    """the counterpart of the refusals: what is not refused goes on to open the device, which the run does not have"""
    r = run_tool(files, "--networks", *extra)
    assert r.returncode == 1 and "lda:" not in r.stderr and "unknown option" not in r.stderr.lower(), r.stderr
    assert "networks" not in r.stderr and "Invalid" not in r.stderr, r.stderr


def test_the_new_symbols_and_the_options_struct(capi):
    L = capi.lib()
    declared = capi.declared_symbols()
    for name in NEW_SYMBOLS:
        assert name in declared and hasattr(L, name), name
    # the network options travel in a struct of their own: aasr_lda_options ends as its callers know it
    assert [f[0] for f in capi.LdaOptions._fields_][-3:] == ["state_gamma", "seconds_scatter", "seconds_features"]
    assert [(n, t) for n, t in capi.LdaNetworkOptions._fields_] == [
        ("networks", ctypes.c_int32), ("viterbi", ctypes.c_int32), ("fw_beam", ctypes.c_double), ("bw_beam", ctypes.c_double),
        ("ac_scale_given", ctypes.c_int32), ("ac_scale", ctypes.c_double)]
    assert ctypes.sizeof(capi.LdaNetworkOptions) == 40
    no = capi.LdaNetworkOptions.defaults()
    assert (no.networks, no.viterbi, no.fw_beam, no.bw_beam, no.ac_scale_given, no.ac_scale) == (0, 0, 0.0, 0.0, 0, 1.0)


def test_without_handles_the_calls_name_themselves(capi, files):
    L = capi.lib()
    assert L.aasr_scatter_accumulate_weighted_dev(None, None, 0, None, None, None, None) == capi.AASR_ERR_INVALID
    assert b"aasr_scatter_accumulate_weighted_dev" in L.aasr_last_error()
    no = capi.LdaNetworkOptions.defaults(networks=1)
    assert L.aasr_run_lda_networks_recipe(None, None, None, None, None, ctypes.byref(no), None) == capi.AASR_ERR_INVALID
    assert b"aasr_run_lda_networks_recipe" in L.aasr_last_error()
    assert L.aasr_run_lda_networks_recipe(None, None, None, None, None, None, None) == capi.AASR_ERR_INVALID
    assert b"aasr_run_lda_recipe" in L.aasr_last_error()                 # no network options: the .phn call's name
    # the host checks as a call of their own
    topo = capi.Topology(str(files / "m.ph"))
    opts = capi.LdaOptions.defaults(module=b"lda", target_dim=2)
    rcp = str(files / "net.rcp").encode()
    assert L.aasr_lda_networks_check(CFG.encode(), topo.handle, rcp, ctypes.byref(opts)) == capi.AASR_OK
    assert L.aasr_lda_networks_check(CFG_NO_MATRIX.encode(), topo.handle, rcp, ctypes.byref(opts)) == capi.AASR_ERR_INVALID
    assert b"module lda has no matrix" in L.aasr_last_error()
    opts.ophn = 1
    assert L.aasr_lda_networks_check(CFG.encode(), topo.handle, rcp, ctypes.byref(opts)) == capi.AASR_ERR_UNSUPPORTED
