"""Write tests/golden/kmeans_sklearn.npz: scikit-learn's KMeans(algorithm="lloyd") on structured images, the
yardstick of the device k-means.  Needs scikit-learn; runs on the host.

    python tools/make_cluster_golden.py

Images: one Gaussian spot per image (width 1.5-3 pixels, log-normal amplitude) centred at one of K mode
positions plus N(0, jitter) jitter, Poisson counts, log1p, fp32 -- numpy's legacy RandomState throughout.  (On
the structureless synthetic batches Lloyd stops after 2-3 iterations with clusters of one member.)

Cases: "proton" 768x56x30, K = 4, init = K data rows; "proton_empty" the same images with one initial centre
set to the constant 50 (empty in iteration 1: one relocation); "neutron" 1024x44x44, K = 6.  Stored per case:
init, scikit-learn's labels, centres, inertia and n_iter_ on the fp64 widening of the images.  A k-means++ case
("pp_*") from tests/cluster_refs.plusplus on the proton images: the draws, the chosen rows.

The tool asserts what makes exact agreement a fair demand and fails otherwise (choose another seed): over every
iteration the smallest relative gap between a row's nearest and second-nearest centre >= 1e-7 and
|shift - threshold| / threshold >= 1e-6; "proton_empty" relocates exactly one cluster; the restatement
(tests/cluster_refs.lloyd) reproduces scikit-learn's labels and n_iter_; the k-means++ case's searchsorted and
potential gaps >= 1e-9 relative.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import cluster_refs as R  # noqa: E402


def spot_images(n, h, w, K, seed, jitter=1.5):
    rs = np.random.RandomState(seed)
    modes = np.stack([rs.uniform(0.2 * h, 0.8 * h, K), rs.uniform(0.2 * w, 0.8 * w, K)], axis=1)
    which = rs.randint(0, K, n)
    centre = modes[which] + rs.normal(0.0, jitter, (n, 2))
    width = rs.uniform(1.5, 3.0, n)
    amp = rs.lognormal(np.log(40.0), 0.5, n)
    yy, xx = np.mgrid[0:h, 0:w]
    r2 = (yy[None] - centre[:, 0, None, None]) ** 2 + (xx[None] - centre[:, 1, None, None]) ** 2
    lam = amp[:, None, None] * np.exp(-0.5 * r2 / width[:, None, None] ** 2)
    return np.log1p(rs.poisson(lam).astype(np.float64)).astype(np.float32), rs


def sklearn_case(images, init, expect_relocated):
    from sklearn.cluster import KMeans
    X = images.reshape(len(images), -1).astype(np.float64)
    km = KMeans(n_clusters=len(init), init=init, n_init=1, algorithm="lloyd", tol=1e-4, max_iter=300).fit(X)
    trace = {}
    labels, centres, inertia, n_iter = R.lloyd(X, init, trace=trace)
    assert np.array_equal(labels, km.labels_) and n_iter == km.n_iter_, "the restatement left scikit-learn"
    assert np.abs(centres - km.cluster_centers_).max() <= 1e-12, np.abs(centres - km.cluster_centers_).max()
    assert abs(inertia - km.inertia_) <= 1e-12 * km.inertia_
    gap, margin, relocated = min(trace["gap"]), min(trace["margin"]), sum(trace["relocated"])
    assert gap >= 1e-7, f"nearest / second-nearest gap {gap:.3g}"
    assert margin >= 1e-6, f"shift / threshold margin {margin:.3g}"
    assert relocated == expect_relocated, f"{relocated} relocations"
    print(f"  n_iter {n_iter}  gap {gap:.3g}  margin {margin:.3g}  relocated {relocated}  inertia {km.inertia_:.6f}")
    return {"init": init, "labels": km.labels_.astype(np.int32), "centres": km.cluster_centers_,
            "inertia": np.float64(km.inertia_), "n_iter": np.int64(km.n_iter_)}


def main():
    out = {}
    proton, rs = spot_images(768, 56, 30, 4, seed=20261021)
    Xp = proton.reshape(len(proton), -1).astype(np.float64)
    init = Xp[rs.choice(len(Xp), 4, replace=False)]
    empty = init.copy()
    empty[2] = 50.0
    neutron, rs_n = spot_images(1024, 44, 44, 6, seed=20261022)
    Xn = neutron.reshape(len(neutron), -1).astype(np.float64)
    init_n = Xn[rs_n.choice(len(Xn), 6, replace=False)]
    out["proton_images"], out["neutron_images"] = proton, neutron
    for name, images, c0, reloc in (("proton", proton, init, 0), ("proton_empty", proton, empty, 1),
                                    ("neutron", neutron, init_n, 0)):
        print(name)
        out.update({f"{name}_{k}": v for k, v in sklearn_case(images, c0, reloc).items()})
    K = 8
    u = np.random.Generator(np.random.Philox(key=[0, 0])).random((K, R.trials(K)))
    trace = {}
    index, _ = R.plusplus(Xp, K, u, trace=trace)
    assert trace["search_gap"] >= 1e-9 and trace["pot_gap"] >= 1e-9, trace
    assert len(set(index.tolist())) == K
    print(f"k-means++  rows {index.tolist()}  search gap {trace['search_gap']:.3g}  potential gap {trace['pot_gap']:.3g}")
    out.update(pp_draws=u, pp_index=index.astype(np.int32))
    path = R.GOLDEN
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
