"""The clip-loader modules by concern: `trainclips` still exports every name it held when it was one file, each the very
object of the module it moved to, and the three host modules import without torch."""
import importlib
import os
import subprocess
import sys

import pytest

from tdeed_amd import trainclips as TC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the module that holds a name now -> the names; for "trainclips" itself the check is that the name is still there.  The old
# private `_ResidentStreams` is not kept: it is `residentstreams.ResidentStreams` now and had no user but evalutil.
HOMES = {
    "cliptable": ["DEFAULT_PAD_LEN", "clip_step", "train_clip_table", "rasterise_labels", "ClipDraws", "JointDraws",
                  "join_clip_tables", "_reaches", "_strides_of"],
    "jpegsets": ["ResidentJpegs", "load_resident_jpegs", "join_resident_jpegs", "batch_tables", "video_tables", "_cut_waves"],
    "streamplan": ["frame_extents", "stream_plan", "stage_batch", "_clip_ranges", "_shard_first", "_round16", "_NO_BYTE"],
    "trainclips": ["load_resident_videos", "ResidentClips", "JointResidentClips", "ResidentJpegClips", "JointResidentJpegClips",
                   "_ClipLoader", "_DeferredMix", "_SlotMix", "_two_parts"],
}


@pytest.mark.parametrize("home", sorted(HOMES))
def test_trainclips_exports_every_name_it_held(home):
    mod = importlib.import_module("tdeed_amd." + home)
    for name in HOMES[home]:
        assert hasattr(TC, name), name
        assert getattr(TC, name) is getattr(mod, name), name
        if home != "trainclips" and callable(getattr(mod, name)):
            assert getattr(mod, name).__module__ == "tdeed_amd." + home, name


def test_resident_streams_is_public_in_its_own_module():
    from tdeed_amd import residentstreams
    assert TC.ResidentStreams is residentstreams.ResidentStreams
    assert residentstreams.ResidentStreams.__module__ == "tdeed_amd.residentstreams"


def test_the_host_modules_import_without_torch():
    code = ("import sys; sys.path.insert(0, %r); import tdeed_amd.cliptable, tdeed_amd.jpegsets, tdeed_amd.streamplan; "
            "bad = [m for m in ('torch', 'tdeed_amd.ops', 'tdeed_amd.feeder', 'tdeed_amd.jpegdev') if m in sys.modules]; "
            "print('loaded', bad); sys.exit(1 if bad else 0)") % ROOT
    done = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True)
    assert done.returncode == 0, done.stdout + done.stderr
