"""CPU checks of the spatial check's classes of pairs, command line and tables (sbayes_amd/spatial.py): bands_from_adjacency and
bands_from_costs against their definitions, the command line's reading of a small costs file and of the x, y columns, and the
tables of a result built from the oracle (tests/_spatial_oracle.py) -- no device call."""
import numpy as np
import pytest

from sbayes_amd import spatial
from tests import _spatial_cases as cases
from tests import _spatial_oracle as orc

NA = spatial.NA


def _costs(n, seed=3):
    rng = np.random.default_rng(seed)
    return spatial.plane_distances(rng.random((n, 2)))


def test_bands_from_adjacency():
    adj = np.zeros((4, 4), dtype=bool)
    adj[0, 1] = adj[1, 0] = adj[2, 3] = adj[3, 2] = adj[1, 1] = True
    band, b = spatial.bands_from_adjacency(adj)
    assert b == 1 and band.dtype == np.uint8 and band.tolist() == [[NA, 0, NA, NA], [0, NA, NA, NA], [NA, NA, NA, 0], [NA, NA, 0, NA]]
    assert orc.check_band(band, b) is None

    class Sparse:                                     # what a scipy.sparse matrix offers
        def toarray(self):
            return adj.astype(np.int8)
    assert np.array_equal(spatial.bands_from_adjacency(Sparse())[0], band)
    adj[0, 2] = True
    with pytest.raises(ValueError, match=r"not symmetric: entry \(0, 2\)"):
        spatial.bands_from_adjacency(adj)
    with pytest.raises(ValueError, match="square matrix"):
        spatial.bands_from_adjacency(np.zeros((3, 4), dtype=bool))


def test_bands_from_costs_by_edges():
    c = np.array([[0, 1, 2, 5], [1, 0, 3, 4], [2, 3, 0, 9], [5, 4, 9, 0]], dtype=np.float64)
    band, b = spatial.bands_from_costs(c, edges=[2, 4])
    # class 0: cost <= 2; class 1: cost in (2, 4]; beyond 4 not counted; the diagonal never
    assert b == 2 and band.tolist() == [[NA, 0, 0, NA], [0, NA, 1, 1], [0, 1, NA, NA], [NA, 1, NA, NA]]
    assert spatial.bands_from_costs(c, edges=[100.0])[0][~np.eye(4, dtype=bool)].tolist() == [0] * 12
    with pytest.raises(ValueError, match="edges must increase"):
        spatial.bands_from_costs(c, edges=[2, 2])
    with pytest.raises(ValueError, match=r"edges must be 1 \.\. 8 bounds"):
        spatial.bands_from_costs(c, edges=list(range(9)))
    with pytest.raises(ValueError, match="exactly one of edges, n_bands and knn"):
        spatial.bands_from_costs(c)
    with pytest.raises(ValueError, match="exactly one of edges, n_bands and knn"):
        spatial.bands_from_costs(c, edges=[1], knn=2)
    c[0, 3] = 6
    with pytest.raises(ValueError, match=r"not symmetric: entry \(0, 3\) = 6.0 differs from \(3, 0\) = 5.0"):
        spatial.bands_from_costs(c, edges=[2, 4])


@pytest.mark.parametrize("b", [1, 3, 8])
def test_bands_from_costs_by_quantiles(b):
    c = _costs(41)
    band, got_b = spatial.bands_from_costs(c, n_bands=b)
    off = ~np.eye(41, dtype=bool)
    assert got_b == b and orc.check_band(band, b) is None and (band[off] < b).all() and (np.diag(band) == NA).all()
    sizes = np.bincount(band[np.triu_indices(41, 1)], minlength=b)
    assert sizes.sum() == 820 and sizes.max() - sizes.min() <= 2              # classes of equal size, up to the quantile's rounding
    # a farther class holds larger costs
    top = [c[off & (band == k)].max() for k in range(b)]
    low = [c[off & (band == k)].min() for k in range(b)]
    assert all(top[k] < low[k + 1] for k in range(b - 1))
    for bad in (0, 9):
        with pytest.raises(ValueError, match=rf"n_bands={bad} out of range"):
            spatial.bands_from_costs(c, n_bands=bad)


def test_bands_from_costs_by_nearest_neighbours():
    c = _costs(30)
    band, b = spatial.bands_from_costs(c, knn=3)
    assert b == 1 and orc.check_band(band, 1) is None and np.array_equal(band, band.T)
    away = c + np.where(np.eye(30, dtype=bool), np.inf, 0)
    for i in range(30):
        nearest = set(np.argsort(away[i], kind="stable")[:3].tolist())
        joined = set(np.nonzero(band[i] == 0)[0].tolist())
        assert nearest <= joined and all(i in set(np.argsort(away[j], kind="stable")[:3].tolist()) for j in joined - nearest)      # the union
    assert 3 * 30 / 2 <= (band == 0).sum() / 2 <= 3 * 30
    assert (spatial.bands_from_costs(c, knn=100)[0][~np.eye(30, dtype=bool)] == 0).all()                                                # k beyond N - 1
    assert spatial.bands_from_costs(np.zeros((1, 1)), knn=6)[0].tolist() == [[NA]]
    with pytest.raises(ValueError, match="knn=0 must be at least 1"):
        spatial.bands_from_costs(c, knn=0)


def test_the_command_line_reads_costs_and_coordinates(tmp_path):
    features = tmp_path / "features.csv"
    features.write_text("id,name,family,x,y,F1\nc,Cc,,3.0,4.0,A\na,Aa,,0.0,0.0,B\nb,Bb,,0.0,1.0,A\n")
    costs = tmp_path / "costs.csv"
    costs.write_text(",a,b,c\na,0,1.5,7\nb,1.5,0,2.5\nc,7,2.5,0\n")                # in another order than the features file
    ids, xy = spatial.read_objects(features)
    assert ids == ["c", "a", "b"] and xy.tolist() == [[3.0, 4.0], [0.0, 0.0], [0.0, 1.0]]
    got = spatial.read_costs(costs, ids)
    assert got.tolist() == [[0, 7, 2.5], [7, 0, 1.5], [2.5, 1.5, 0]]
    with pytest.raises(ValueError, match="no row or no column for object 'd'"):
        spatial.read_costs(costs, ["a", "d"])
    ap = spatial.parser()
    common = [str(features), "states.csv", "stats.txt", "clusters.txt"]
    args = ap.parse_args(common + ["--costs", str(costs), "--edges", "2", "3"])
    band, b = spatial.bands_of_args(args, ids, xy)
    assert b == 2 and band.tolist() == [[NA, NA, 1], [NA, NA, 0], [1, 0, NA]]
    # without --costs: plane distances of the x, y columns (c-a 5, c-b sqrt(18), a-b 1), and by default the 6 nearest neighbours
    args = ap.parse_args(common + ["--bands", "3"])
    assert args.costs is None and args.out_features.name == "spatial_features.tsv" and args.out_objects.name == "spatial_objects.tsv"
    assert (args.burnin, args.seed, args.confounders) == (0.1, 0, [])
    band, b = spatial.bands_of_args(args, ids, xy)
    assert b == 3 and band.tolist() == [[NA, 2, 1], [2, NA, 0], [1, 0, NA]]
    band, b = spatial.bands_of_args(ap.parse_args(common), ids, xy)
    assert b == 1 and band.tolist() == [[NA, 0, 0], [0, NA, 0], [0, 0, NA]]
    band, b = spatial.bands_of_args(ap.parse_args(common + ["--knn", "1"]), ids, xy)
    assert band.tolist() == [[NA, NA, 0], [NA, NA, 0], [0, 0, NA]]
    with pytest.raises(SystemExit):
        ap.parse_args(common + ["--knn", "2", "--bands", "3"])
    help_text = " ".join(ap.format_help().split())                              # (argparse wraps the lines)
    assert "plane distances" in help_text and "x, y columns" in help_text and "conservative" in help_text


def _result(name):
    x, ns, band, b, y, want = cases.case(name)
    fields = {k: want[k].astype(np.int32) for k in ("agree_obs", "comparable_obs", "local_agree_obs", "local_comparable_obs")}
    fields.update({k: want[k] for k in orc.ACCUMULATORS})
    return spatial.SpatialResult(total_obs=want["total_obs"], n_replicates=want["n_replicates"], total_rep=want["total_rep"], **fields), want


def test_the_tables_of_a_result(tmp_path):
    res, want = _result("n65")
    b, f, n, t = 3, 17, 65, 5
    header, rows = res.table()
    assert header == ["band", "feature", "agree", "comparable", "share", "p_predictive", "mean_replicated", "sd_replicated", "z"]
    assert len(rows) == b * f and rows[0][1].startswith("F")
    keys = [(r[5], -r[8] if r[8] == r[8] else np.inf) for r in rows]
    assert keys == sorted(keys)
    p = res.p_value()
    assert p.shape == (b, f) and ((p >= 0) & (p <= 1)).all() and np.array_equal(p, (want["f_greater"] + 0.5 * want["f_equal"]) / t)
    for row in rows[:4] + rows[-4:]:
        k, at = row[0], int(row[1][1:]) - 1
        assert row[2:4] == [int(want["agree_obs"][k, at]), int(want["comparable_obs"][k, at])] and row[5] == p[k, at]
        assert row[6] == want["agree_rep"][:, k, at].mean() and abs(row[7] - want["agree_rep"][:, k, at].std()) <= 1e-9 * max(1.0, row[7])
    assert res.worst(3) == rows[:3] or all(a[:4] == c[:4] for a, c in zip(res.worst(3), rows[:3]))
    oheader, orows = res.object_table([f"lang{i}" for i in range(n)])
    assert oheader[1] == "object" and len(orows) == b * n and orows[0][1].startswith("lang")
    # the totals: mean and sd exactly from total_rep, ties count half
    assert np.array_equal(res.mean("total"), want["total_rep"].mean(axis=0)) and np.allclose(res.sd("total"), want["total_rep"].std(axis=0), rtol=1e-12)
    assert np.array_equal(res.p_value("total"), (want["t_greater"] + 0.5 * want["t_equal"]) / t)
    assert np.allclose(res.sd("object"), want["local_agree_rep"].std(axis=0), rtol=1e-9, atol=1e-9)
    share = res.share_obs()
    assert np.isnan(share[:, 16]).all() and np.nanmax(share) <= 1.0                # feature 16 is observed nowhere
    z = res.z()
    assert np.isnan(z[res.sd() == 0]).all() and np.isfinite(z[res.sd() > 0]).all()
    with pytest.raises(ValueError, match="16 names for 17 features"):
        res.table(["x"] * 16)
    with pytest.raises(ValueError, match="kind='pair' is none of"):
        res.p_value("pair")
    res.write_tables(tmp_path / "f.tsv", tmp_path / "o.tsv")
    lines = (tmp_path / "f.tsv").read_text().splitlines()
    assert lines[0].split("\t") == header and len(lines) == 1 + b * f and lines[1].split("\t")[:2] == [str(rows[0][0]), rows[0][1]]
    assert len((tmp_path / "o.tsv").read_text().splitlines()) == 1 + b * n
    res.write_tables(objects_path=tmp_path / "only.tsv")
    assert (tmp_path / "only.tsv").exists()


def test_a_result_without_replicates():
    res, want = _result("n63")
    res.n_replicates, res.total_rep = 0, np.zeros((0, 8), dtype=np.int64)
    for k in orc.ACCUMULATORS:
        setattr(res, k, np.zeros_like(want[k]))
    assert np.isnan(res.p_value()).all() and np.isnan(res.sd()).all() and np.isnan(res.sd("total")).all() and np.isnan(res.z("total")).all()
