"""Writes the fixtures of the diffusion and pole filter tests and prints the measured figures that tests/polefilter_cases.py records.

    python tools/make_polefilter_goldens.py            # tests/golden/polefilter_<case>.npz, polefilter_diff_{a,b}.npz; prints E_TAB, E_REF, INCREMENT

Per case: float64 inputs (T, U, V; 2 planes), sig, the cutoff index and the fp64 oracle's V1, QV1 and V2 results.  The 70-channel
diff_lap2d_filt result on g24x144 goes into two files (its input is polefilter_cases.diff_tensor()).  E_ref is the largest
difference between the fp64 oracle and the same chain in np.longdouble; E_tab the same for the tables.  numpy only."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import polefilter_cases as PC  # noqa: E402
import polefilter_oracle as PO  # noqa: E402


def up(x):
    """x rounded up in the third digit"""
    if x == 0:
        return 0.0
    e = int(np.floor(np.log10(x))) - 2
    return float(np.ceil(x / 10.0 ** e) * 10.0 ** e)


def run(G, T, Uw, Vw, sig, i):
    return {"V1": PO.polefilt_lap2d_V1(G, T, PC.SUBSTEPS["V1"], sig, i), "QV1": PO.polefilt_lap2d_QV1(G, T, PC.SUBSTEPS["QV1"], sig, i),
            "V2": PO.polefilt_lap2d_V2(G, Uw, Vw, PC.SUBSTEPS["V2"], sig, i)}


def main():
    os.makedirs(PC.GOLD, exist_ok=True)
    e_tab, e_ref, inc = {}, {}, {}
    for name in PC.SYNTHESIS_CASES:
        G, GL = PC.geometry(name), PC.geometry(name, np.longdouble)
        e_tab[name] = up(max(float(np.abs(G.tab[k] - GL.tab[k]).max()) for k in G.tab))
        if name not in PC.FILTER_CASES:
            continue
        i = PC.FILTER_CASES[name][5]
        assert PO.cutoff_index(G.nlon) == i, (name, PO.cutoff_index(G.nlon))
        sig = PO.sigmoid_ramp(G.nlat)
        T = PC.temperature(name, PC.GOLD_PLANES)
        Uw, Vw = PC.wind(name, PC.GOLD_PLANES)
        got, ref = run(G, T, Uw, Vw, sig, i), run(GL, T, Uw, Vw, sig, i)
        e_ref[(name, "V1")] = up(float(np.abs(got["V1"] - ref["V1"]).max()))
        e_ref[(name, "QV1")] = up(float(np.abs(got["QV1"] - ref["QV1"]).max()))
        e_ref[(name, "V2")] = up(float(max(np.abs(got["V2"][0] - ref["V2"][0]).max(), np.abs(got["V2"][1] - ref["V2"][1]).max())))
        Tl, Ul, Vl = PO.polfilt_fft(T, i), PO.polfilt_fft(Uw, i), PO.polfilt_fft(Vw, i)      # the increment of the sub-steps alone
        inc[(name, "V1")] = float(np.abs(got["V1"] - Tl).max())
        inc[(name, "QV1")] = float(np.abs(got["QV1"] - Tl).max())
        inc[(name, "V2")] = float(max(np.abs(got["V2"][0] - Ul).max(), np.abs(got["V2"][1] - Vl).max()))
        np.savez(os.path.join(PC.GOLD, f"polefilter_{name}.npz"), T=T, U=Uw, V=Vw, sig=sig, cutoff=np.int64(i), V1=got["V1"], QV1=got["QV1"],
                 V2u=got["V2"][0], V2v=got["V2"][1])
        print(name, {k[1]: (e_ref[k], round(inc[k], 3)) for k in e_ref if k[0] == name}, flush=True)
    name = PC.DIFF_CASE
    G, GL = PC.geometry(name), PC.geometry(name, np.longdouble)
    B, sig, i = PC.diff_tensor(), PO.sigmoid_ramp(G.nlat), PC.FILTER_CASES[name][5]
    got, ref = PO.diff_lap2d_filt(G, B, sig, i), PO.diff_lap2d_filt(GL, B, sig, i)
    np.savez(os.path.join(PC.GOLD, PC.DIFF_FILES[0]), expected=got[:35], sig=sig, cutoff=np.int64(i))
    np.savez(os.path.join(PC.GOLD, PC.DIFF_FILES[1]), expected=got[35:])
    print("E_TAB =", e_tab)
    print("E_REF =", e_ref)
    print("INCREMENT =", {k: round(v, 3) for k, v in inc.items()})
    print("E_REF_DIFF, INCREMENT_DIFF =", up(float(np.abs(got - ref).max())), round(float(np.abs(got - PO.polfilt_fft(B, i)).max()), 3))


if __name__ == "__main__":
    main()
