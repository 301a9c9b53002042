"""The device stage-1 reader (kmahip_ingest_dev_*) as far as a machine without a GPU can see it: the entry points exist, and inputs
the reader does not cover are refused before it makes any HIP call (so these pass where no device exists)."""
import os
import re

import pytest

from kma_amd import binding

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ING = os.path.join(ROOT, "tests", "golden", "ingest")
ENTRY = ["kmahip_ingest_dev_open", "kmahip_ingest_dev_next", "kmahip_ingest_dev_status", "kmahip_ingest_dev_phred_scale",
         "kmahip_ingest_dev_counts", "kmahip_ingest_dev_close", "kmahip_session_upload_dev"]
EXTRA = ["kmahip_ingest_dev_handed_back", "kmahip_ingest_dev_timing", "kmahip_ingest_dev_copy_out"]


def test_header_declares_and_library_exports_the_device_reader():
    header = open(os.path.join(ROOT, "include", "kmahip.h")).read()
    lib = binding.lib()
    for name in ENTRY + EXTRA:
        assert re.search(r"\b%s\s*\(" % name, header), f"kmahip.h does not declare {name}"
        assert hasattr(lib, name), f"libkmahip.so does not export {name}"
    assert hasattr(binding, "IngestDev")


@pytest.mark.parametrize("name,why", [("p33gz.fq.gz", "gzip"), ("wrap.fa", "FASTA")])
def test_inputs_the_device_reader_does_not_cover_are_refused_without_a_device(name, why):
    with pytest.raises(binding.KmaHipError) as e:
        binding.IngestDev(os.path.join(ING, name))
    assert "kmahip error -3" in str(e.value) and why in str(e.value)          # KMAHIP_EFORMAT, and the reason by name


def test_a_refused_mate_file_refuses_the_pair():
    with pytest.raises(binding.KmaHipError) as e:
        binding.IngestDev(os.path.join(ING, "m1.fq"), os.path.join(ING, "p33gz.fq.gz"))
    assert "kmahip error -3" in str(e.value)


def test_a_missing_file_is_an_io_error():
    with pytest.raises(binding.KmaHipError) as e:
        binding.IngestDev(os.path.join(ING, "does_not_exist.fq"))
    assert "kmahip error -2" in str(e.value)                                    # KMAHIP_EIO


def test_session_upload_dev_refuses_null_arguments():
    assert binding.lib().kmahip_session_upload_dev(None, None) == -1             # KMAHIP_EINVAL, no device touched
