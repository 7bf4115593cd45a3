"""CPU check of the index mapping of the wide memory phases of tfk_cr_factor (csrc/tf_cr_io.h): the g++
harness tests/cr_io_host runs it for b = 3 ... 8, chunk lengths 1 ... 16 and 256 / 512 threads against the
loops it replaces (same LDS slots loaded once from the same record entries, the two parts of a diagonal
entry in one thread, same slots zeroed once, same share of the next level, the staged record read from where
it was put)."""
from tests.cr_io_host import build_cr_io_host


def test_mapping_covers_what_the_loops_cover():
    status, out = build_cr_io_host.run()
    assert status == 0 and out.strip().endswith("0 failures"), out
