"""Provenance rule of dstd-gcn_amd/Makefile: experiment flags (DEFS) build only
under a variant name, so libdstd_gcn.so is always the default-flag build.
Dry runs (make -n): nothing is compiled or written."""
import os
import subprocess

from conftest import ROOT


def _make_n(*args):
    # -B: print every command even where a built library is up to date
    return subprocess.run(["make", "-n", "-B", "-C", os.path.join(ROOT, "dstd-gcn_amd"), *args],
                          capture_output=True, text=True)


def test_defs_need_a_variant_name():
    r = _make_n("DEFS=-DDSTD_STAMPS")
    assert r.returncode != 0
    assert "VARIANT" in r.stderr
    r = _make_n("VARIANT=stamps", "DEFS=-DDSTD_STAMPS")
    assert r.returncode == 0, r.stderr
    assert "libdstd_gcn_stamps.so" in r.stdout and "-DDSTD_STAMPS" in r.stdout
    r = _make_n()
    assert r.returncode == 0, r.stderr
    assert "-o libdstd_gcn.so" in r.stdout and "-DDSTD" not in r.stdout
