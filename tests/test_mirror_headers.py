"""CPU tests of the drop-in boundary's C++ mirror headers (host/include): what a caller written
against the reference's include/SOM.hpp & co. needs in order to recompile."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "variational-self-organizing-maps_amd", "host", "include")


def _errors(src, std="c++23", extra=()):
    r = subprocess.run(["g++", f"-std={std}", "-fsyntax-only", "-I", INC, *extra, src],
                       capture_output=True, text=True)
    return [l for l in r.stderr.splitlines() if re.search(r"\berror\b", l)], r.stderr


def test_mirror_declares_reference_members(tmp_path):
    """a caller's translation unit that touches the members SOM.hpp:139-171 declares (incl.
    getSizeFromFile, the ARG_* argv indices and std::strcmp through the SOM.hpp include chain)"""
    src = tmp_path / "caller.cpp"
    src.write_text(r'''
#include "SOM.hpp"
#include "SqliteDataLoader.hpp"
int use(int argc, char **argv, Som &som, DataSet &data)
{
    if (argc > ARG_SOM_WEIGHT_DECAY_FUNCTION && std::strcmp(argv[ARG_SETTING], "-t") == 0) {
        som.randomInitialize(1, (float)std::atof(argv[ARG_SOM_INIT_SIGMA]));
        som.train(data, (size_t)std::atoi(argv[ARG_SOM_EPOCHS]), std::atof(argv[ARG_SOM_ETA0]),
                  std::atof(argv[ARG_SOM_ETA_DEC]), std::atof(argv[ARG_SOM_SIGMA0]), std::atof(argv[ARG_SOM_SIGMA_DEC]),
                  Som::WeigthDecayFunction::BatchMap);
        som.save(argv[ARG_SOM_FILE]);
    }
    Eigen::VectorXf v = som.getSizeFromFile(argv[ARG_SOM_FILE]);
    (void)argv[ARG_DB_FILE]; (void)argv[ARG_SOM_HEIGHT]; (void)argv[ARG_SOM_WIDTH];
    return som.measureSimilarity(&data, std::atoi(argv[ARG_ALLOWED_STD_DEV]), (size_t)std::atoi(argv[ARG_MIN_BMU_HITS]))
           + (int)v.size();
}
''')
    errs, full = _errors(str(src), std="c++20")
    assert not errs, full
