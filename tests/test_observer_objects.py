"""What a code object holds: an observer's holds the kernels of its kind and no others, the model's own holds
no observer's, and each is cached against the headers it is compiled from (cross-compiled for gfx950; no
GPU)."""
import os
import re
import shutil
import subprocess

import pytest

from oracle import corpus
from triflow_amd import Model, codegen, compilers, probes

#: kind -> (its header, its kernels, its lowering)
KINDS = {
    "probe": ("tf_probe.h", ["tfk_probe_partial", "tfk_probe_final"],
              lambda m, d: codegen.lower_probes(m, d, ["integral", "argmax"])),
    "record": ("tf_record.h", ["tfk_record"], codegen.lower_records),
    "stat": ("tf_stat.h", ["tfk_stat"], codegen.lower_statistics),
    "spectrum": ("tf_spectrum.h", ["tfk_spectrum_partial", "tfk_spectrum_final"], codegen.lower_spectra),
    "extrema": ("tf_extrema.h", ["tfk_extrema_count", "tfk_extrema_write"], codegen.lower_extrema),
    "histogram": ("tf_histogram.h", ["tfk_hist_partial", "tfk_hist_final"], codegen.lower_histograms),
}
OBSERVER_PREFIXES = ("tfk_probe", "tfk_record", "tfk_stat", "tfk_spectrum", "tfk_extrema", "tfk_hist")
_MODEL = []


def _model():
    if not _MODEL:
        _MODEL.append(Model(*corpus.model_args("M2_diff"), hold_compilation=True))
    return _MODEL[0]


def _kernel_symbols(hsaco):
    out = subprocess.run(["/opt/rocm/lib/llvm/bin/llvm-readelf", "-s", hsaco], capture_output=True, text=True,
                         check=True).stdout
    return set(re.findall(r"\btfk_\w+", out))


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_an_observer_code_object_holds_the_kernels_of_its_kind_and_no_others(kind, tmp_path):
    header, kernels, lower = KINDS[kind]
    model = _model()
    block, _ = lower(model, [probes.discretise(model, "U"), probes.discretise(model, "k * dxxU")])
    hsaco = compilers.build_observer_code_object(model, block, kind)
    usage = compilers.resource_usage(hsaco)
    assert sorted(usage) == sorted(kernels)
    for kernel in kernels:
        assert usage[kernel]["ScratchSize"] == 0 and usage[kernel]["VGPRs"] > 0, (kernel, usage[kernel])
    assert _kernel_symbols(hsaco) == set(kernels)
    # the model's own code object holds no observer's kernel
    plain, _ = compilers.build_code_object(model)
    assert not [k for k in compilers.resource_usage(plain) if k.startswith(OBSERVER_PREFIXES)]
    assert not [s for s in _kernel_symbols(plain) if s.startswith(OBSERVER_PREFIXES)]
    # the stamp lists: the kind's header names the kind's code objects, not the solver's
    assert header in compilers._OBSERVER_SKELETON[kind] and header not in compilers._SKELETON
    assert compilers._OBSERVER_SKELETON[kind][:4] == ("tf_args.h", "tf_math.h", "tf_layout.h", "tf_node.h")
    assert "tf_layout.h" in compilers._SKELETON and "tf_node.h" not in compilers._SKELETON
    for other in set(KINDS) - {kind}:
        assert header not in compilers._OBSERVER_SKELETON[other]
    # an edit of the header (of a copy of it) changes the kind's stamp, so its tags, and no one else's
    csrc = str(tmp_path / "csrc")
    shutil.copytree(compilers.CSRC, csrc)
    assert compilers._skeleton_stamp(kind, csrc) == compilers._skeleton_stamp(kind)
    with open(os.path.join(csrc, header), "a") as f:
        f.write("// edited\n")
    assert compilers._skeleton_stamp(kind, csrc) != compilers._skeleton_stamp(kind)
    assert compilers._skeleton_stamp(None, csrc) == compilers._skeleton_stamp()
    for other in set(KINDS) - {kind}:
        assert compilers._skeleton_stamp(other, csrc) == compilers._skeleton_stamp(other)
    meta = hsaco[:-len(".hsaco")] + ".json"
    with open(meta) as f:
        assert '"kind": "%s"' % kind in f.read()


def test_a_cache_entry_is_held_to_the_stamp_of_its_kind(tmp_path, monkeypatch):
    """evict_stale_cache: an entry stays while the stamp of its own kind and the compiler are what they were;
    an entry of another stamp, of an unknown kind or without the key goes."""
    import json
    monkeypatch.setattr(compilers, "CACHE_DIR", str(tmp_path))
    entries = {"a": dict(kind="model", skeleton=compilers._skeleton_stamp()),
               "b": dict(kind="spectrum", skeleton=compilers._skeleton_stamp("spectrum")),
               "c": dict(kind="spectrum", skeleton=compilers._skeleton_stamp()),          # (the solver's stamp)
               "d": dict(kind="model", skeleton=compilers._skeleton_stamp("spectrum")),
               "e": dict(skeleton=compilers._skeleton_stamp()),                            # (written before the key)
               "f": dict(kind="spectre", skeleton=compilers._skeleton_stamp())}
    for name, meta in entries.items():
        for ext in (".hsaco", ".hip"):
            (tmp_path / ("model_%s%s" % (name, ext))).write_text("")
        (tmp_path / ("model_%s.json" % name)).write_text(json.dumps(dict(meta, hipcc=compilers.hipcc_version())))
    assert compilers.evict_stale_cache() == 4 * 3
    assert sorted(p.name for p in tmp_path.iterdir() if p.suffix == ".hsaco") == ["model_a.hsaco", "model_b.hsaco"]
