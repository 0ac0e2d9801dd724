"""`alphabeta --simulate .. --sim-replicates R`: without noise the run's usual files are the bytes of the run without the
flag; simulation.txt and simulation_raw.npy beside them; miscalls and dropouts change the pedigree; the flag combinations
it refuses, by their messages."""
import numpy as np
import pytest

from test_sim_cli_gpu import LISTS, alphabeta

pytestmark = pytest.mark.gpu
SIM = ("--simulate", "2e-3,5e-3", "--sim-sites", 50_001, "--seed", 77, "-i", 20, *LISTS)
HEADER = ("alpha_true;beta_true;sites;replicates;replicates_ok;mean_alpha;mean_beta;sd_alpha;sd_beta;ci_alpha_0.025;ci_alpha_0.975;"
          "ci_beta_0.025;ci_beta_0.975")


def test_replicates_without_noise_and_with_it(tmp_path):
    one, four, noisy = tmp_path / "one", tmp_path / "four", tmp_path / "noisy"
    for d in (one, four, noisy):
        d.mkdir()
    r = alphabeta(*SIM, "-o", one)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    r = alphabeta(*SIM, "--sim-replicates", 4, "-o", four)
    assert r.returncode == 0 and "Replicates with a finite fit: 4 of 4" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    for name in ("analysis.txt", "pedigree.txt", "raw.npy"):
        assert (one / name).read_bytes() == (four / name).read_bytes(), name
    assert not (one / "simulation.txt").exists() and not (one / "simulation_raw.npy").exists()
    lines = (four / "simulation.txt").read_text().splitlines()
    assert len(lines) == 2 and lines[0] == HEADER
    row = lines[1].split(";")
    assert row[:5] == ["0.002", "0.005", "50001", "4", "4"] and len(row) == 13
    raw = np.load(four / "simulation_raw.npy")
    assert raw.shape == (4, 7) and raw.dtype == np.float64 and np.isfinite(raw).all()
    values = [float(x) for x in row[5:]]
    for k in range(2):           # the analysis of those rows: a mean of four doubles, summed in whichever order
        assert abs(values[k] - raw[:, k].mean()) <= 8.0 * np.spacing(abs(values[k]))
    assert values[4] <= values[0] <= values[5] and values[6] <= values[1] <= values[7]
    r = alphabeta(*SIM, "--sim-replicates", 4, "--sim-miscall", 0.02, "--sim-dropout", 0.1, "-o", noisy)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert (noisy / "pedigree.txt").read_bytes() != (one / "pedigree.txt").read_bytes()
    assert np.load(noisy / "simulation_raw.npy").shape == (4, 7)
    assert (noisy / "simulation.txt").read_text().splitlines()[1].split(";")[3] == "4"


def test_refused_combinations(tmp_path):
    r = alphabeta("--sim-replicates", 4, *LISTS, "-o", tmp_path)
    assert r.returncode == 2 and "belong to --simulate" in r.stderr, r.stderr
    for flag in ("--sim-miscall", "--sim-dropout", "--sim-starts"):
        r = alphabeta(flag, 1, *LISTS, "-o", tmp_path)
        assert r.returncode == 2 and "belong to --simulate" in r.stderr, r.stderr
    sim = ("--simulate", "2e-3,5e-3", "--sim-sites", 1000, *LISTS, "-o", tmp_path)
    r = alphabeta(*sim, "--sim-miscall", 0.1)
    assert r.returncode == 2 and "belong to --sim-replicates" in r.stderr, r.stderr
    r = alphabeta(*sim, "--sim-replicates", 2, "--sim-miscall", 1.5)
    assert r.returncode == 2 and "--sim-miscall expects a probability in [0, 1]" in r.stderr, r.stderr
    r = alphabeta(*sim, "--sim-replicates", 2, "--sim-dropout", -0.1)
    assert r.returncode == 2 and "--sim-dropout expects a probability in [0, 1]" in r.stderr, r.stderr
    r = alphabeta(*sim, "--sim-replicates", 0)
    assert r.returncode == 2 and "--sim-replicates expects a positive number" in r.stderr, r.stderr
    r = alphabeta(*sim, "--sim-replicates", 2, "--sim-starts", 0)
    assert r.returncode == 2 and "--sim-starts expects a positive number" in r.stderr, r.stderr
    r = alphabeta("--simulate", "2e-3,5e-3", "--sim-sites", 1 << 20, "--sim-replicates", (1 << 14) + 1, *LISTS, "-o", tmp_path)
    assert r.returncode == 2 and "--sim-replicates x --sim-sites lies above 2^34" in r.stderr, r.stderr
    assert not list(tmp_path.iterdir())
