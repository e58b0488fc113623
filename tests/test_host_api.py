"""The C++ host API (include/rustsasa_amd.hpp: SASAOptions<Level>::process) driven
through rustsasa_amd/lib/sasa_host_cli, checked against an independent Python
restatement of the reference's level logic (src/options.rs) on top of the oracle."""
import json
import os
import subprocess

import numpy as np
import pytest

import structio as sio
from oracle import pyoracle as po

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
from conftest import ensure_built

CLI = ensure_built()
FIXTURES = ["example.cif", "1jcd.pdb", "151L_H3.pdb", "bad_seqadv_1A06.pdb", "2drt.pdb"]
POLAR = {"SER", "THR", "CYS", "ASN", "GLN", "TYR"}


def run_cli(level, name, *opts, expect_rc=0):
    p = subprocess.run([CLI, level, sio.data_path(name), *opts], capture_output=True, text=True)
    assert p.returncode == expect_rc, (p.returncode, p.stdout[:300], p.stderr[:300])
    return json.loads(p.stdout) if p.stdout.strip() else None


def f32_seq_sum(values):
    t = np.float32(0)
    for v in values:
        t = np.float32(t + np.float32(v))
    return float(t)


def residues_in_order(atoms):
    """chains (first-appearance order) -> residues (first-appearance order) -> atom lists."""
    chains, order = {}, []
    for a in atoms:
        if a.chain not in chains:
            chains[a.chain] = ({}, [])
            order.append(a.chain)
        res, rorder = chains[a.chain]
        key = (a.resseq, a.icode)
        if key not in res:
            res[key] = []
            rorder.append(key)
        res[key].append(a)
    out = []
    for c in order:
        res, rorder = chains[c]
        for key in rorder:
            out.append((c, key, res[key]))
    return out


def n_model_atoms(atoms):
    """Atoms of the model the reader builds: atoms without an alternate location count once per conformer of a
    residue that has alternate locations (structio.conformers)."""
    return sum(len(c[2]) for _, _, ratoms in residues_in_order(atoms) for c in sio.conformers(ratoms))


def expected(name, n_points=100, include_hetatms=False, vdw_fallback=False, include_hydrogens=False,
             radii_from_occupancy=False, radii_table=None, path=None):
    atoms = sio.read_structure(path or sio.data_path(name))
    tab = sio.parse_protor(sio.data_path("protor.config"))
    sel, res_offsets, res_meta, chain_of_res = [], [0], [], []
    for chain, (resseq, icode), ratoms in residues_in_order(atoms):
        conf_name, _, conf_atoms = sio.conformers(ratoms)[0]  # `residue.conformers().next()`, options.rs:162,255
        for a in conf_atoms:
            if (a.element == "H" and not include_hydrogens) or (a.hetero and not include_hetatms):
                continue
            if radii_from_occupancy:
                r = a.occupancy                                  # options.rs:83-84
            else:
                r = (radii_table or {}).get((a.resname, a.name))  # utils.rs:45-53: the custom table first
                if r is None:
                    r = tab.get((a.resname, a.name))
                if r is None:
                    assert vdw_fallback, (a.resname, a.name)
                    r = sio.VDW[a.element]
            sel.append((a, r))
        res_offsets.append(len(sel))
        res_meta.append((resseq, icode, conf_name, chain))
    x = np.array([a.x for a, _ in sel], np.float64).astype(np.float32)
    y = np.array([a.y for a, _ in sel], np.float64).astype(np.float32)
    z = np.array([a.z for a, _ in sel], np.float64).astype(np.float32)
    r = np.array([rr for _, rr in sel], np.float32)
    ids = np.array([a.serial for a, _ in sel], np.uint64)
    atom = po.calculate_sasa_internal(x, y, z, r, ids, 1.4, n_points, 8)
    res = po.residue_sums(atom, np.array(res_offsets, np.uint32))
    return atom, res, res_meta


@pytest.mark.parametrize("name", FIXTURES)
def test_reader_counts_match_independent_parser(name):
    atoms = sio.read_structure(sio.data_path(name))
    got = run_cli("parse", name)
    assert got["atoms"] == n_model_atoms(atoms)
    assert got["chains"] == len({a.chain for a in atoms})
    assert got["residues"] == len({(a.chain, a.resseq, a.icode) for a in atoms})


def test_no_gpu_is_a_loud_engine_error():
    import rustsasa_amd
    if rustsasa_amd.device_count() > 0:
        pytest.skip("GPU present")
    got = run_cli("atom", "1jcd.pdb", expect_rc=2)
    assert got["error"] == 7 and "no usable HIP device" in got["message"]


def test_radius_missing_is_reported_before_the_hot_path():
    # HETATM ligands have no ProtOr entry: RadiusMissing unless vdW fallback is allowed
    got = run_cli("atom", "2drt.pdb", "--include-hetatms", expect_rc=2)
    assert got["error"] == 3 and "Radius not found for residue" in got["message"]


@pytest.mark.gpu
@pytest.mark.parametrize("name", FIXTURES)
def test_atom_and_residue_levels(name):
    atom, res, meta = expected(name)
    got = run_cli("atom", name)["Atom"]
    assert len(got) == len(atom)
    assert np.array_equal(np.array(got, np.float32), atom)
    got_res = run_cli("residue", name)["Residue"]
    assert len(got_res) == len(meta)
    for g, v, (resseq, icode, resname, chain) in zip(got_res, res, meta):
        assert g["serial_number"] == resseq and g["insertion_code"] == icode
        assert g["name"] == resname and g["chain_id"] == chain
        assert g["is_polar"] == (resname in POLAR)
        assert np.float32(g["value"]) == v
    # residues made only of HETATM records are reported with 0.0 (reference tests/io.rs:165-224)
    hetero_only = [g for g, (_, _, resname, _) in zip(got_res, meta) if resname == "HOH"]
    assert all(g["value"] == 0.0 for g in hetero_only)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["example.cif", "1jcd.pdb"])
def test_chain_and_protein_levels(name):
    atom, res, meta = expected(name)
    chains = []
    for (_, _, _, c) in meta:
        if c not in chains:
            chains.append(c)
    got = run_cli("chain", name)["Chain"]
    assert [g["name"] for g in got] == chains
    # atoms of a chain are contiguous: sequential f32 sum over them (options.rs:304-308)
    offs = [0]
    a_all = sio.read_structure(sio.data_path(name))
    kept_chain = [a.chain for a in a_all if not a.hetero and a.element != "H"]
    for c in chains:
        offs.append(offs[-1] + sum(1 for k in kept_chain if k == c))
    for g, b, e in zip(got, offs[:-1], offs[1:]):
        assert np.float32(g["value"]) == np.float32(f32_seq_sum(atom[b:e]))
    prot = run_cli("protein", name)["Protein"]
    assert np.float32(prot["global_total"]) == np.float32(f32_seq_sum(atom))
    polar = f32_seq_sum([v for v, m in zip(res, meta) if m[2] in POLAR])
    non_polar = f32_seq_sum([v for v, m in zip(res, meta) if m[2] not in POLAR])
    assert np.float32(prot["polar_total"]) == np.float32(polar)
    assert np.float32(prot["non_polar_total"]) == np.float32(non_polar)


@pytest.mark.gpu
def test_reference_literals_within_their_own_tolerance():
    """tests/units.rs:58,76,89 (+-1500): example.cif, 1A06 and 151L protein totals."""
    for name, literal in (("example.cif", 20268.004), ("bad_seqadv_1A06.pdb", 14466.709),
                          ("151L_H3.pdb", 9558.812)):
        prot = run_cli("protein", name)["Protein"]
        assert abs(prot["global_total"] - literal) <= 1500.0
    hi = run_cli("protein", "example.cif", "--n-points", "960")["Protein"]
    assert abs(hi["global_total"] - 20131.227) <= 1500.0
    assert abs(hi["polar_total"] - 4279.8906) <= 1500.0
    assert abs(hi["non_polar_total"] - 15999.43) <= 1500.0


@pytest.mark.gpu
def test_options_hetatms_with_vdw_fallback_and_points():
    atom, _, _ = expected("2drt.pdb", n_points=200, include_hetatms=True, vdw_fallback=True)
    got = run_cli("atom", "2drt.pdb", "--include-hetatms", "--allow-vdw-fallback", "--n-points", "200")["Atom"]
    assert np.array_equal(np.array(got, np.float32), atom)


# ---- the reader's decimal parser and directory mode (process_files) ------------------

def test_decimal_parser_equals_strtod():
    rng = np.random.default_rng(1)
    toks = []
    for _ in range(4000):
        toks.append("%8.3f" % rng.uniform(-999, 9999))                       # PDB coordinate field
        toks.append(repr(round(float(rng.normal(scale=10.0 ** int(rng.integers(-3, 6)))), int(rng.integers(0, 9)))))
        toks.append("%d" % rng.integers(-10 ** 9, 10 ** 9))
        toks.append("%.*f" % (int(rng.integers(0, 18)), rng.uniform(-1e4, 1e4)))  # long mantissas
        toks.append("%.6e" % rng.normal(scale=1e3))                          # exponents -> strtod path
    toks += ["0", "-0.0", ".5", "5.", "+3.25", "00012.500", "1e400", "abc", "1.2.3"]
    p = subprocess.run([CLI, "decimal"], input=" ".join(t.strip() for t in toks), capture_output=True,
                       text=True)
    assert p.returncode == 0
    lines = p.stdout.strip().split("\n")
    assert len(lines) == len(toks)
    bad = [(t, l) for t, l in zip(toks, lines) if l.split()[0] != l.split()[1]]
    assert not bad, bad[:5]


def _write_variant(src, dst, rng):
    """Rigidly moved copy of a PDB fixture (columns 31-54 rewritten)."""
    import bench_workloads as bw
    rot = bw._random_rotation(rng)
    shift = rng.uniform(-30, 30, size=3)
    lines = open(sio.data_path(src)).read().split("\n")
    pts = np.array([[float(l[30:38]), float(l[38:46]), float(l[46:54])] for l in lines
                    if l.startswith(("ATOM  ", "HETATM"))])
    c = pts.mean(axis=0)
    with open(dst, "w") as f:
        for l in lines:
            if l.startswith(("ATOM  ", "HETATM")):
                v = (np.array([float(l[30:38]), float(l[38:46]), float(l[46:54])]) - c) @ rot.T + shift
                l = l[:30] + "%8.3f%8.3f%8.3f" % tuple(v) + l[54:]
            f.write(l + "\n")


def _make_file_set(tmp_path, n=12):
    rng = np.random.default_rng(9)
    paths = []
    for i in range(n):
        src = ["1jcd.pdb", "151L_H3.pdb", "bad_seqadv_1A06.pdb", "2drt.pdb"][i % 4]
        dst = str(tmp_path / f"v{i:03d}_{src}")
        _write_variant(src, dst, rng)
        paths.append(dst)
    paths.insert(3, sio.data_path("example.cif"))
    paths.insert(5, str(tmp_path / "does_not_exist.pdb"))
    # a structure whose radius lookup fails (unknown residue name) must only fail itself
    broken = str(tmp_path / "unknown_residue.pdb")
    with open(broken, "w") as f:
        f.write("ATOM      1  N   XYZ A   1      11.104   6.134  -6.504  1.00  0.00           N  \n")
    paths.insert(8, broken)
    lst = str(tmp_path / "files.txt")
    open(lst, "w").write("\n".join(paths) + "\n")
    return paths, lst


def test_process_files_reports_errors_per_file(tmp_path):
    paths, lst = _make_file_set(tmp_path, 4)
    p = subprocess.run([CLI, "files", "residue", lst, "--threads", "3"], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[:500]
    got = json.loads(p.stdout)
    assert got["n_files"] == len(paths)
    errs = {i: r.get("error") for i, r in enumerate(got["results"]) if "error" in r}
    i_missing = next(i for i, p_ in enumerate(paths) if p_.endswith("does_not_exist.pdb"))
    i_broken = next(i for i, p_ in enumerate(paths) if p_.endswith("unknown_residue.pdb"))
    assert errs[i_missing] == 7 and errs[i_broken] == 3   # unreadable file / RadiusMissing
    import rustsasa_amd
    if rustsasa_amd.device_count() == 0:            # no GPU: the good files fail loudly too
        assert got["n_ok"] == 0 and all(r.get("error") == 7 for i, r in enumerate(got["results"])
                                        if i not in (i_missing, i_broken))


@pytest.mark.gpu
@pytest.mark.parametrize("batch,workers", [(0, 0), (5, 0), (3, 3)])
def test_process_files_matches_oracle(tmp_path, batch, workers):
    """Chunks of `batch` files go through a queue to `workers` GPU worker threads, each with its own
    context (here all on device 0; one per GPU in production): results keep the input order."""
    paths, lst = _make_file_set(tmp_path, 12)
    p = subprocess.run([CLI, "files", "residue", lst, "--threads", "4", "--batch", str(batch), "--full",
                        "--workers", str(workers), "--devices", "1"], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[:500]
    got = json.loads(p.stdout)
    assert got["n_ok"] == len(paths) - 2
    for i, (path, r) in enumerate(zip(paths, got["results"])):
        if path.endswith(("does_not_exist.pdb", "unknown_residue.pdb")):
            assert "error" in r
            continue
        # `expected` resolves names under tests/golden/data; give it the absolute path instead
        atoms_backup = sio.data_path
        try:
            sio.data_path = lambda name, _p=path: _p if name == "__file__" else atoms_backup(name)
            _, res, _ = expected("__file__")
        finally:
            sio.data_path = atoms_backup
        assert np.array_equal(np.array(r, np.float32), res), path
    # protein level through the same batch path
    p = subprocess.run([CLI, "files", "protein", lst, "--full"], capture_output=True, text=True)
    prot = json.loads(p.stdout)["results"]
    single = run_cli("protein", "example.cif")["Protein"]
    i_cif = paths.index(sio.data_path("example.cif"))
    assert np.array_equal(np.array(prot[i_cif], np.float32),
                          np.array([single["global_total"], single["polar_total"],
                                    single["non_polar_total"]], np.float32))


@pytest.mark.gpu
@pytest.mark.parametrize("workers", [0, 1])
def test_process_files_companion_context_runs_with_the_callers_settings(tmp_path, workers):
    """With one context and more files than a chunk holds, process_files puts a second (cached) context on the same
    GPU beside it; chunks go to whichever worker is free, so the companion must carry the caller's pulp lane
    count (it decides which points take the remainder rule) - results would otherwise depend on the run.  Twice in
    one process: the second call finds the cached companion."""
    paths, lst = _make_file_set(tmp_path, 12)
    p = subprocess.run([CLI, "files", "residue", lst, "--threads", "4", "--batch", "4", "--full", "--simd-width", "4",
                        "--workers", str(workers), "--calls", "2"], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[:500]
    got = json.loads(p.stdout)
    assert got["worker_simd_widths"] == [4, 4], got["worker_simd_widths"]
    assert got["n_ok"] == len(paths) - 2
    # (on these files the oracle's values are the same for every lane count: the widths above are the check)
    i_cif = paths.index(sio.data_path("example.cif"))
    _, res, _ = expected("example.cif")
    assert np.array_equal(np.array(got["results"][i_cif], np.float32), res)


@pytest.mark.gpu
def test_process_files_with_radii_from_occupancy_reads_the_occupancies(tmp_path):
    """Directory mode skips the conversion of occupancy / b-factor columns unless an option needs them
    (prepare_text's skip_occupancy_and_bfactor argument): with radii from the occupancy column the values must be the
    single-file results of the same option."""
    paths = [sio.data_path(n) for n in ("1jcd.pdb", "151L_H3.pdb", "example.cif")]
    lst = str(tmp_path / "files.txt")
    open(lst, "w").write("\n".join(paths) + "\n")
    p = subprocess.run([CLI, "files", "residue", lst, "--full", "--read-radii-from-occupancy"], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[:500]
    got = json.loads(p.stdout)
    assert got["n_ok"] == len(paths)
    for path, r in zip(paths, got["results"]):
        single = run_cli("residue", os.path.basename(path), "--read-radii-from-occupancy")["Residue"]
        assert np.array_equal(np.array(r, np.float32), np.array([x["value"] for x in single], np.float32)), path


def _prepare_json(path, level, fast, *opts):
    p = subprocess.run([CLI, "prepare-fast" if fast else "prepare-general", str(path), "--level", str(level), *opts],
                       capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[:300]
    return json.loads(p.stdout)


def test_directory_modes_short_cut_equals_the_general_reader(tmp_path):
    """process_files reads plain PDB files straight into the kept atoms (prepare.cpp fast_pdb_prepare) and leaves
    everything else to the general reader + selection.  Both must hand the GPU the same atoms (bit patterns of x, y, z,
    radius; ids), the same segment ends and the same result metadata - on the fixtures, under the options the
    reference tests, and on mutants that hit each of the short cut's exits (alternate locations, chains and residues
    that come back, descending numbers, short records, missing elements and radii, several models)."""
    rng = np.random.default_rng(5)
    names = ["151L_H3.pdb", "bad_seqadv_1A06.pdb", "1jcd.pdb", "2drt.pdb", "freesasa/2gpi.pdb", "freesasa/4c1a.pdb"]
    option_sets = [(), ("--include-hetatms", "--allow-vdw-fallback"), ("--include-hydrogens", "--allow-vdw-fallback"),
                   ("--read-radii-from-occupancy",)]
    n_fast = n_cases = 0

    def compare(path, label):
        nonlocal n_fast, n_cases
        for level in (0, 1, 2, 3):
            for opts in option_sets:
                a, b = _prepare_json(path, level, True, *opts), _prepare_json(path, level, False, *opts)
                n_fast += a.pop("fast")
                b.pop("fast")
                n_cases += 1
                assert a == b, (label, level, opts, len(a["atoms"]), len(b["atoms"]), a["error"], b["error"])

    for name in names:
        compare(sio.data_path(name), name)
        lines = open(sio.data_path(name)).read().split("\n")
        atom_idx = [i for i, l in enumerate(lines) if l.startswith(("ATOM  ", "HETATM"))]
        for m in range(14):
            mut = list(lines)
            i = int(rng.choice(atom_idx[5:-5]))
            kind = m % 14
            if kind == 0:   mut[i] = mut[i][:16] + "A" + mut[i][17:]                       # an alternate location
            elif kind == 1: mut[i] = mut[i][:21] + "Z" + mut[i][22:]                       # a one-atom chain in the middle
            elif kind == 2: mut[i], mut[i + 1] = mut[i + 1], mut[i]                         # two records swapped
            elif kind == 3: mut[i] = mut[i][:40]                                            # a short record
            elif kind == 4: mut[i] = mut[i][:76] + "  " + mut[i][78:]                       # no element symbol
            elif kind == 5: mut[i] = mut[i][:12] + " XX " + mut[i][16:]                     # an atom name without a radius
            elif kind == 6: mut.insert(i, "ENDMDL"); mut.insert(i + 1, "MODEL        2")    # a second model
            elif kind == 7: mut[i] = mut[i][:22] + "%4d" % 1 + mut[i][26:]                  # a residue number that goes back
            elif kind == 8: mut[i] = mut[i][:17] + "GLY" + mut[i][20:]                      # another name inside a residue
            elif kind == 9: mut[i] = mut[i][:26] + "B" + mut[i][27:]                        # an insertion code
            elif kind == 10: mut[i] = mut[i][:6] + "  abc" + mut[i][11:]                    # a serial number that is not one
            elif kind == 11: mut[i] = "HETATM" + mut[i][6:]                                 # a HETATM inside a residue
            elif kind == 12: mut[i] = mut[i][:20] + "x" + mut[i][21:]                       # a character in column 21
            elif kind == 13: mut = mut[:i] + mut[atom_idx[2]:atom_idx[8]] + mut[i:]         # an early residue repeated later
            path = tmp_path / f"mut_{os.path.basename(name)}_{m}.pdb"
            path.write_text("\n".join(mut))
            compare(path, f"{name} mutant {kind}")
    assert n_fast > 40 and n_cases - n_fast > 40, (n_fast, n_cases)  # both routes were exercised


def _pdb_to_mmcif(pdb_path, quote_names=True):
    """The ATOM / HETATM records of a PDB file as an AlphaFold-style mmCIF text (one `_atom_site` loop, a row per line,
    the column order of tests/golden/data/example.cif).  Test input only: no attempt at a complete mmCIF file."""
    cols = ["group_PDB", "id", "type_symbol", "label_atom_id", "label_alt_id", "label_comp_id", "label_asym_id", "auth_asym_id",
            "label_entity_id", "label_seq_id", "auth_seq_id", "pdbx_PDB_ins_code", "Cartn_x", "Cartn_y", "Cartn_z", "occupancy",
            "B_iso_or_equiv", "pdbx_formal_charge", "pdbx_PDB_model_num"]
    rows, model = [], 1
    for l in open(pdb_path):
        l = l.rstrip("\n")
        if l.startswith("MODEL"):
            model = int(l[10:14] or 1)
        if not l.startswith(("ATOM  ", "HETATM")) or len(l) < 54:
            continue
        name = l[12:16].strip()
        if quote_names and "'" in name:
            name = '"%s"' % name
        dot = lambda t: t.strip() or "."  # noqa: E731
        rows.append(" ".join([l[:6].strip(), dot(l[6:11]), dot(l[76:78]), name or ".", dot(l[16:17]), dot(l[17:20]), dot(l[21:22]),
                              dot(l[21:22]), "1", dot(l[22:26]), dot(l[22:26]), dot(l[26:27]), dot(l[30:38]), dot(l[38:46]),
                              dot(l[46:54]), dot(l[54:60]), dot(l[60:66]), "?", str(model)]))
    return "data_test\n#\nloop_\n" + "".join("_atom_site.%s\n" % c for c in cols) + "\n".join(rows) + "\n#\n"


def test_directory_modes_mmcif_short_cut_equals_the_general_reader(tmp_path):
    """The same for mmCIF text (prepare.cpp fast_cif_prepare): the reference's AlphaFold fixture, the PDB fixtures
    rewritten as `_atom_site` loops, and mutants of them that hit the short cut's exits - an alternate location, a chain
    that comes back, rows swapped, a row with a token too few or too many, no element symbol, an atom without a radius,
    a second model, a residue number that goes back, a second name inside a residue, an insertion code, a serial number
    that is not one, a HETATM inside a residue, '?' for a coordinate, an early residue repeated later, a second loop; and
    rows that the aligned-column row splitter must not mis-split: tabs, quoted names, other column positions, a row of
    more than 256 bytes, a byte above 127, a token wider than its column."""
    rng = np.random.default_rng(11)
    texts = {"example.cif": open(sio.data_path("example.cif")).read()}
    for name in ["151L_H3.pdb", "bad_seqadv_1A06.pdb", "1jcd.pdb", "2drt.pdb", "freesasa/2gpi.pdb", "freesasa/4c1a.pdb"]:
        texts[name] = _pdb_to_mmcif(sio.data_path(name))
    option_sets = [(), ("--include-hetatms", "--allow-vdw-fallback"), ("--include-hydrogens", "--allow-vdw-fallback"),
                   ("--read-radii-from-occupancy",)]
    n_fast = n_cases = 0

    def compare(path, label, levels=(0, 1, 2, 3), sets=option_sets):
        nonlocal n_fast, n_cases
        for level in levels:
            for opts in sets:
                a, b = _prepare_json(path, level, True, *opts), _prepare_json(path, level, False, *opts)
                n_fast += a.pop("fast")
                b.pop("fast")
                n_cases += 1
                assert a == b, (label, level, opts, len(a["atoms"]), len(b["atoms"]), a["error"], b["error"])

    for name, text in texts.items():
        base = tmp_path / (os.path.basename(name) + ".cif")
        base.write_text(text)
        compare(base, name)
        lines = text.split("\n")
        atom_idx = [i for i, l in enumerate(lines) if l.startswith(("ATOM ", "HETATM "))]
        for kind in range(23):
            mut = list(lines)
            i = int(rng.choice(atom_idx[5:-5]))
            f = mut[i].split()

            def put(k, v, row=None):
                g = list(f if row is None else row)
                g[k] = v
                return " ".join(g)
            if kind == 0:   mut[i] = put(4, "A")                                        # an alternate location
            elif kind == 1: mut[i] = put(7, "Z")                                        # a one-atom chain in the middle
            elif kind == 2: mut[i], mut[i + 1] = mut[i + 1], mut[i]                     # two rows swapped
            elif kind == 3: mut[i] = " ".join(f[:-1])                                   # a token too few
            elif kind == 4: mut[i] = put(2, "?")                                        # no element symbol
            elif kind == 5: mut[i] = put(3, "XX")                                       # an atom name without a radius
            elif kind == 6: mut[i:] = [put(18, "2", l.split()) if l.startswith(("ATOM ", "HETATM ")) else l for l in mut[i:]]  # a second model
            elif kind == 7: mut[i] = put(10, "1")                                       # a residue number that goes back
            elif kind == 8: mut[i] = put(5, "GLY" if f[5] != "GLY" else "ALA")          # another name inside a residue
            elif kind == 9: mut[i] = put(11, "B")                                       # an insertion code
            elif kind == 10: mut[i] = put(1, "abc")                                     # a serial number that is not one
            elif kind == 11: mut[i] = put(0, "HETATM")                                  # a HETATM inside a residue
            elif kind == 12: mut[i] = put(12, "?")                                      # no x coordinate
            elif kind == 13: mut = mut[:i] + mut[atom_idx[2]:atom_idx[8]] + mut[i:]     # an early residue repeated later
            elif kind == 14: mut[i] = mut[i] + " extra"                                 # a token too many
            elif kind == 15: mut = mut[:i] + ["#", "loop_", "_atom_site.Cartn_x", "_atom_site.Cartn_y", "_atom_site.Cartn_z",
                                               "_atom_site.label_atom_id", "_atom_site.label_comp_id", "1.0 2.0 3.0 CA ALA"] + ["#"]  # rows cut short, a second loop
            # rows the aligned-column splitter must hand to the character-wise tokenizer, or split differently
            elif kind == 16: mut[i] = mut[i].replace(" ", "\t", 3)                      # tabs between tokens
            elif kind == 17: mut[i] = put(3, '"%s"' % f[3])                             # a quoted atom name
            elif kind == 18: mut[i] = put(3, "'%s'" % f[3])                             # ... in single quotes
            elif kind == 19: mut[i] = "   " + mut[i].replace(" ", "   ", 5) + "    "    # other column positions, blanks around
            elif kind == 20: mut[i] = put(16, "1." + "0" * 300)                         # a row of more than 256 bytes
            elif kind == 21: mut[i] = put(5, "\u00c5LA")                                # a byte above 127
            elif kind == 22: mut[i] = put(1, str(10 ** 7 + i))                          # a wider token: the columns shift
            path = tmp_path / f"mut_{os.path.basename(name)}_{kind}.cif"
            path.write_text("\n".join(mut))
            compare(path, f"{name} mutant {kind}", (1, 2), option_sets[:2] if kind % 2 else option_sets[2:])
    assert n_fast > 60 and n_cases - n_fast > 60, (n_fast, n_cases)  # both routes were exercised


def _element_forms_pdb(nameless):
    """Thirteen hand-written records whose element columns take every form the element rule distinguishes.  Atoms of
    ALA / GLY carry ProtOr names (a radius whatever the symbol says), the HETATM records do not (van-der-Waals radius of
    the WHOLE upper-cased symbol).  `nameless`: one more record without a symbol whose name has no letter - no element."""
    rows = [  # record, name, residue, number, element columns 77-78
        ("ATOM", "N", "ALA", 1, " N"),
        ("ATOM", "CA", "ALA", 1, " H"),      # hydrogen
        ("ATOM", "C", "ALA", 1, " h"),       # hydrogen, lower case
        ("ATOM", "O", "ALA", 1, "HG"),       # two letters that start with H: mercury, helium, holmium - not hydrogen
        ("ATOM", "CB", "ALA", 1, "HE"),
        ("ATOM", "N", "GLY", 2, "HO"),
        ("ATOM", "CA", "GLY", 2, "Zn"),      # mixed case
        ("ATOM", "C", "GLY", 2, " C"),       # (the mmCIF text gives this one the three-character symbol ZN2)
        ("ATOM", "O", "GLY", 2, "  "),       # no symbol: the name's first letter, O
        ("ATOM", "1H", "GLY", 2, "  "),      # no symbol: the name's first LETTER, H - hydrogen
        ("HETATM", "ZN", "ZN", 3, "Zn"),     # no ProtOr name: the look-up takes ZN
        ("HETATM", "HG", "HG", 4, "HG"),     # ... and HG, 2.45 - H alone would be 1.20
        ("HETATM", "X1", "UNK", 5, " h"),    # a hetero hydrogen
    ]
    if nameless:
        rows.insert(9, ("ATOM", "123", "GLY", 2, "  "))
    return "".join("%-6s%5d %-4s %3s A%4d    %8.3f%8.3f%8.3f  0.75 10.00          %2s  \n" %
                   (rec, k + 1, name if len(name) == 4 else " " + name, res, seq, 1.5 * k, 0.25 * k, -0.5 * k, el)
                   for k, (rec, name, res, seq, el) in enumerate(rows)) + "END\n"


@pytest.mark.parametrize("fmt", ["pdb", "cif"])
def test_element_forms_decide_the_same_on_both_routes(tmp_path, fmt):
    """One element rule behind both short cuts (prepare.cpp LightModel::keep_atom) and the general reader's
    set_element + selection: the symbol's first character in upper case, hydrogen only when the symbol is that one
    character, without a symbol the first letter of the name, and the van-der-Waals look-up with the whole upper-cased
    symbol.  Short cut and general reader must agree on atoms, segment ends, model and error; the short cut must
    TAKE the file where every atom has an element and leave the one with a letterless name to the general reader,
    which reports the missing element.  The kept-atom counts are written out by hand."""
    option_sets = {(): 7,                                                # ATOM records that are not hydrogen (H, h, 1H)
                   ("--allow-vdw-fallback",): 7,
                   ("--include-hydrogens", "--allow-vdw-fallback"): 10,  # every ATOM record
                   ("--include-hetatms", "--allow-vdw-fallback"): 9}     # + ZN and HG; the hetero h stays out
    for nameless in (False, True):
        path = tmp_path / f"forms_{int(nameless)}.pdb"
        path.write_text(_element_forms_pdb(nameless))
        if fmt == "cif":
            lines = _pdb_to_mmcif(path).split("\n")
            i = next(k for k, l in enumerate(lines) if l.startswith("ATOM 8 C C "))
            lines[i] = lines[i].replace("ATOM 8 C C ", "ATOM 8 ZN2 C ", 1)
            path = tmp_path / f"forms_{int(nameless)}.cif"
            path.write_text("\n".join(lines))
        for opts, n_kept in option_sets.items():
            for level in (1, 2):
                a, b = _prepare_json(path, level, True, *opts), _prepare_json(path, level, False, *opts)
                took = a.pop("fast")
                assert b.pop("fast") is False
                assert a == b, (nameless, opts, level, len(a["atoms"]), len(b["atoms"]), a["error"], b["error"])
                if nameless:
                    assert took is False and a["error"] == 1, (opts, level, took, a["error"])  # ElementMissing
                else:
                    assert took is True and a["error"] == 0, (opts, level, took, a["error"])
                    assert len(a["atoms"]) == n_kept, (opts, level, len(a["atoms"]))
                    assert a["seg_end"][-1] == n_kept and len(a["seg_end"]) == (1 if level == 2 else 5)
                    if "--include-hetatms" in opts:  # the look-up took the whole symbol: ZN and HG, not Z (none) or H (1.20)
                        radii = [float.fromhex(r[3]) for r in a["atoms"][-2:]]
                        assert radii == [float(np.float32(2.39)), float(np.float32(2.45))], radii


def _cif_without_x(tmp_path):
    """An mmCIF file whose `_atom_site` loop has no Cartn_x column: the general reader throws on it."""
    bad = tmp_path / "no_x.cif"
    bad.write_text(_pdb_to_mmcif(sio.data_path("1jcd.pdb")).replace("_atom_site.Cartn_x\n", "_atom_site.Cartn_q\n"))
    return str(bad)


def test_a_reader_that_throws_leaves_nothing_behind_on_its_thread(tmp_path):
    """Directory mode asks the readers to skip occupancies and b-factors; that request is an argument of the call
    (host_internal.h read_pdb_text / read_mmcif_text), so a reader that throws cannot leave it switched on for the
    thread's later callers.  `sasa_host_cli after-throw` reads the throwing file in directory mode on its own thread,
    then opens a good file on the same thread: the occupancies must be the file's, not the default 1.0.  No GPU."""
    good = tmp_path / "occ.pdb"
    occs = [0.25, 0.5, 0.75, 0.3]
    good.write_text("".join("ATOM  %5d  CA  ALA A%4d    %8.3f%8.3f%8.3f%6.2f%6.2f           C  \n" % (k + 1, k + 1, 3.8 * k, 0.0, 0.0, o, 20.0)
                            for k, o in enumerate(occs)) + "END\n")
    p = subprocess.run([CLI, "after-throw", _cif_without_x(tmp_path), str(good)], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[:500]
    assert json.loads(p.stdout) == occs


@pytest.mark.gpu
def test_process_files_goes_on_unharmed_after_a_reader_that_throws(tmp_path):
    """The same in directory mode itself: one parse thread reads a file the general reader throws on, then two good
    ones - they must get their single-file values, the first its own error."""
    paths = [_cif_without_x(tmp_path), sio.data_path("1jcd.pdb"), sio.data_path("example.cif")]
    lst = str(tmp_path / "files.txt")
    open(lst, "w").write("\n".join(paths) + "\n")
    p = subprocess.run([CLI, "files", "residue", lst, "--threads", "1", "--full"], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[:500]
    got = json.loads(p.stdout)
    assert got["n_ok"] == 2 and got["results"][0] == {"error": 7}
    for path, r in zip(paths[1:], got["results"][1:]):
        single = run_cli("residue", os.path.basename(path))["Residue"]
        assert np.array_equal(np.array(r, np.float32), np.array([x["value"] for x in single], np.float32)), path


def test_fixed_column_decimals_equal_the_general_parser(tmp_path):
    """The PDB reader takes %8.3f / %6.2f fields through a fixed-layout fast path (integer / power of ten, as Clinger's
    exact case) and everything else through the general parser / strtod: both must give the double Python's float()
    gives, for well-formed fields, shifted points, exponents, signs without digits, negative zero.  No GPU: the
    selection (`select --read-radii-from-occupancy`) prints x, y, z and the occupancy-as-radius as f32."""
    coords = ["  -0.000", "9999.999", "-999.999", "   0.001", "  1.2345", " 1.5e+01", "   -.500", "     12.", "  12.000",
              "-123.456", "   7.100", "0012.500", "  +3.250", "    3.25", " 100.0  "]
    occs = ["  1.00", " -0.50", "  0.5 ", "  .750", " 12.34", "1.0e-1", "  2.  ", "  0.00", " -0.00", "  9.99"]
    lines = []
    for k, c in enumerate(coords):
        o = occs[k % len(occs)]
        y, z = coords[(k + 3) % len(coords)], coords[(k + 7) % len(coords)]
        lines.append("ATOM  %5d  CA  ALA A%4d    %s%s%s%s  0.00           C  " % (k + 1, k + 1, c, y, z, o))
    path = tmp_path / "fields.pdb"
    path.write_text("\n".join(lines) + "\nEND\n")
    p = subprocess.run([CLI, "select", str(path), "--read-radii-from-occupancy"], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[:500]
    atoms = json.loads(p.stdout)["atoms"]
    assert len(atoms) == len(coords)
    for k, a in enumerate(atoms):
        want = [coords[k], coords[(k + 3) % len(coords)], coords[(k + 7) % len(coords)], occs[k % len(occs)]]
        for got, text in zip(a[:4], want):
            w = np.float32(float(text))
            assert np.float32(got) == w, (k, text, got)  # (the JSON number "-0" reads back as an int: no sign check on zeros)


# ---- writers (reference src/utils/io.rs) ---------------------------------------------

@pytest.mark.parametrize("name", ["1jcd.pdb", "151L_H3.pdb", "2drt.pdb"])
def test_pdb_writer_round_trip(name):
    p = subprocess.run([CLI, "rewrite", sio.data_path(name)], capture_output=True, text=True)
    assert p.returncode == 0
    src = [l.rstrip("\n") for l in open(sio.data_path(name)) if l.startswith(("ATOM  ", "HETATM"))]
    out = [l for l in p.stdout.split("\n") if l.startswith(("ATOM  ", "HETATM"))]
    assert len(src) == len(out)
    # chains are written grouped (pdbtbx merges records of one chain id), so compare as sets
    # of the fixed columns 1-66 + element
    key = lambda l: (l[:66], l[76:78].strip())  # noqa: E731
    assert sorted(map(key, src)) == sorted(map(key, out))


@pytest.mark.gpu
def test_bfactor_write_back(tmp_path):
    out = str(tmp_path / "res.pdb")
    got = run_cli("residue", "1jcd.pdb", "--bfactor-out", out)["Residue"]
    atoms = sio.read_pdb(out)
    bf = {}
    for l in open(out):
        if l.startswith(("ATOM  ", "HETATM")):
            bf.setdefault((l[21], int(l[22:26])), set()).add(float(l[60:66]))
    assert len(atoms) == 1238
    for g in got:
        vals = bf[(g["chain_id"], g["serial_number"])]
        assert len(vals) == 1 and abs(vals.pop() - g["value"]) <= 0.005 + 1e-6
    # atom level with filtered atoms cannot be mapped back (the reference would index out of range)
    p = subprocess.run([CLI, "atom", sio.data_path("1jcd.pdb"), "--bfactor-out", out], capture_output=True, text=True)
    assert p.returncode == 3 and "cannot be mapped back" in p.stderr


@pytest.mark.parametrize("name", ["1jcd.pdb", "example.cif", "freesasa/4c1a.pdb"])
def test_structure_copies_and_moves_keep_their_nodes(name):
    """The model's nodes live in a pool the Structure owns: copies, moved-to objects and vector elements must stay
    whole after their source is gone (sasa_host_cli model-selftest; tools/fuzz_reader.py --asan runs it sanitized)."""
    p = subprocess.run([CLI, "model-selftest", sio.data_path(name)], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    assert json.loads(p.stdout)["ok"] is True


@pytest.mark.gpu
def test_json_shape_matches_serde():
    p = subprocess.run([CLI, "residue", sio.data_path("2drt.pdb")], capture_output=True, text=True)
    text = p.stdout.strip()
    assert text.startswith('{"Residue":[{"serial_number":') and text.endswith("]}")
    first = json.loads(text)["Residue"][0]
    assert list(first.keys()) == ["serial_number", "insertion_code", "value", "name", "is_polar", "chain_id"]
    prot = subprocess.run([CLI, "protein", sio.data_path("2drt.pdb")], capture_output=True, text=True).stdout
    assert list(json.loads(prot)["Protein"].keys()) == ["global_total", "polar_total", "non_polar_total"]


# ---- files with alternate locations (the reference's quality set, tests/quality.rs) -----------
ALTLOC = ["2gpi", "3w7y", "3uc7", "3kyz", "4oxx", "3zsj"]
RMSE_GATE = 43.99 + 20.0   # RMSE_BASELINE + TOLERANCE, reference tests/quality.rs:17-18,225


def _altloc_count(name):
    return sum(1 for a in sio.read_structure(sio.data_path(name)) if a.altloc not in ("", " "))


@pytest.mark.parametrize("pid", ALTLOC)
def test_altloc_reader_counts_match_independent_parser(pid):
    name = f"freesasa/{pid}.pdb"
    assert _altloc_count(name) > 0          # the fixture really exercises alternate locations
    atoms = sio.read_structure(sio.data_path(name))
    got = run_cli("parse", name)
    assert got["atoms"] == n_model_atoms(atoms) >= len(atoms)  # (shared atoms count once per conformer)
    assert got["chains"] == len({a.chain for a in atoms})
    assert got["residues"] == len({(a.chain, a.resseq, a.icode) for a in atoms})


@pytest.mark.gpu
@pytest.mark.parametrize("pid", ALTLOC)
def test_first_conformer_selection_on_altloc_files(pid):
    """A residue contributes its FIRST conformer only (reference src/options.rs:162,255:
    `residue.conformers().next()`): the first (residue name, alt-loc) pair met in file order, plus - in a
    residue with alternate locations - the atoms without one, which belong to every conformer (this is what
    reproduces the reference's own RMSE of 43.99 on its whole FreeSASA set: tools/check_quality_set.py).
    The C++ reader must select exactly the atoms the independent Python reader selects, give them
    the same radii, and do so deterministically."""
    name = f"freesasa/{pid}.pdb"
    atom, res, meta = expected(name)
    n_all = sum(1 for a in sio.read_structure(sio.data_path(name)) if not a.hetero and a.element != "H")
    assert len(atom) < n_all                # alternate conformers were dropped
    first = run_cli("atom", name)["Atom"]
    again = run_cli("atom", name)["Atom"]
    assert first == again
    assert len(first) == len(atom)
    assert np.array_equal(np.array(first, np.float32), atom)
    got_res = run_cli("residue", name)["Residue"]
    assert [g["serial_number"] for g in got_res] == [m[0] for m in meta]
    assert np.array_equal(np.array([g["value"] for g in got_res], np.float32), res)


@pytest.mark.gpu
def test_altloc_files_meet_the_reference_quality_gate():
    """The reference's own gate on this kind of input (tests/quality.rs:225): RMSE of the chain
    totals against FreeSASA's (Lee & Richards, a different algorithm) at most 63.99 A^2."""
    ours, theirs = [], []
    for pid in ALTLOC:
        ref = json.load(open(sio.data_path(f"freesasa/{pid}.json")))
        want = {c["label"]: c["area"]["total"] for r in ref["results"] for s in r["structure"] for c in s["chains"]}
        got = {c["name"]: c["value"] for c in run_cli("chain", f"freesasa/{pid}.pdb")["Chain"]}
        common = sorted(set(want) & set(got))
        assert common, (pid, want.keys(), got.keys())
        ours += [got[k] for k in common]
        theirs += [want[k] for k in common]
    rmse = float(np.sqrt(np.mean((np.array(ours) - np.array(theirs)) ** 2)))
    assert len(ours) >= len(ALTLOC)
    assert rmse <= RMSE_GATE, rmse


# ---- host options the reference tests and the reader semantics behind them ---------------------------------
# (tests/quality.rs:340-442 radii from occupancy; src/utils/consts.rs:31-81 + src/utils.rs:40-56 custom radii
# file; src/options.rs:166 hydrogens: 12 of the reference's 88 quality files carry them, here 4c1a)

def _with_radii_in_occupancy(src, dst):
    """tests/quality.rs:262-334: every atom's occupancy becomes its ProtOr radius (vdW radius where the table has none)."""
    tab = sio.parse_protor(sio.data_path("protor.config"))
    out = []
    for line in open(src):
        if line.startswith(("ATOM", "HETATM")):
            r = tab.get((line[17:20].strip(), line[12:16].strip()))
            if r is None:
                r = sio.VDW.get(line[76:78].strip().upper(), 2.0)
            line = line[:54] + f"{r:6.2f}" + line[60:]
        out.append(line)
    open(dst, "w").write("".join(out))


RADII_FILE = """name: custom
types:
BIGC 2.25 apolar
SMALLO 1.25 polar
atoms:
ALA CB BIGC
GLY O SMALLO
LEU CD1 BIGC
XYZ Q BIGC
"""


def _select(path, *opts):
    p = subprocess.run([CLI, "select", path, *opts], capture_output=True, text=True)
    assert p.returncode == 0, (p.stdout[:300], p.stderr[:300])
    d = json.loads(p.stdout)
    a = d["atoms"]
    cols = [np.array([v[k] for v in a], np.float32) for k in range(4)]
    ids = np.array([int(v[4]) for v in a], np.uint64)
    return cols, ids, d


def _expected_selection(path, **kw):
    atoms = sio.read_structure(path)
    tab = sio.parse_protor(sio.data_path("protor.config"))
    sel = []
    for chain, _, ratoms in residues_in_order(atoms):
        for a in sio.conformers(ratoms)[0][2]:
            if (a.element == "H" and not kw.get("include_hydrogens")) or (a.hetero and not kw.get("include_hetatms")):
                continue
            if kw.get("radii_from_occupancy"):
                r = a.occupancy
            else:
                r = (kw.get("radii_table") or {}).get((a.resname, a.name))
                if r is None:
                    r = tab.get((a.resname, a.name))
                if r is None:
                    r = sio.VDW[a.element]
            sel.append((a, r, chain))
    return sel


OPTION_CASES = [
    ("freesasa/4c1a.pdb", ["--include-hydrogens", "--allow-vdw-fallback"], dict(include_hydrogens=True)),
    ("freesasa/4c1a.pdb", [], {}),
    ("freesasa/3kyz.pdb", ["--include-hetatms", "--allow-vdw-fallback"], dict(include_hetatms=True)),
    ("1jcd.pdb", ["--read-radii-from-occupancy"], dict(radii_from_occupancy=True)),
    ("freesasa/2gpi.pdb", ["--read-radii-from-occupancy"], dict(radii_from_occupancy=True)),
    ("1jcd.pdb", ["--radii-file"], dict(radii_table=True)),
    ("example.cif", ["--radii-file"], dict(radii_table=True)),
]


def _case(tmp_path, name, opts, kw):
    path = sio.data_path(name)
    kw = dict(kw)
    opts = list(opts)
    if kw.get("radii_from_occupancy"):
        dst = str(tmp_path / os.path.basename(name))
        _with_radii_in_occupancy(path, dst)
        path = dst
    if kw.get("radii_table"):
        cfg = tmp_path / "custom.config"
        cfg.write_text(RADII_FILE)
        opts.append(str(cfg))
        kw["radii_table"] = {("ALA", "CB"): 2.25, ("GLY", "O"): 1.25, ("LEU", "CD1"): 2.25}
    return path, opts, kw


@pytest.mark.parametrize("name,opts,kw", OPTION_CASES)
def test_selection_under_reference_tested_options(tmp_path, name, opts, kw):
    """No GPU: the atoms, radii and chains the C++ host API hands to the hot path (`sasa_host_cli select`)
    against the independent Python reader, for the options the reference's own tests exercise."""
    path, opts, kw = _case(tmp_path, name, opts, kw)
    (x, y, z, r), ids, d = _select(path, *opts)
    want = _expected_selection(path, **kw)
    assert len(x) == len(want) > 0
    assert np.array_equal(x, np.array([a.x for a, _, _ in want], np.float64).astype(np.float32))
    assert np.array_equal(y, np.array([a.y for a, _, _ in want], np.float64).astype(np.float32))
    assert np.array_equal(z, np.array([a.z for a, _, _ in want], np.float64).astype(np.float32))
    assert np.array_equal(r, np.array([rr for _, rr, _ in want], np.float64).astype(np.float32))
    if kw.get("include_hydrogens"):
        assert any(a.element == "H" for a, _, _ in want)
    if kw.get("radii_table"):
        assert np.any(r == np.float32(2.25))
    # chains: ids in file order, contiguous ranges
    chains = []
    for _, _, c in want:
        if not chains or chains[-1][0] != c:
            chains.append([c, 0])
        chains[-1][1] += 1
    assert [c for c, _ in chains] == [c for c, e, b in zip(d["chains"], d["chain_end"], [0] + d["chain_end"]) if e > b]
    assert len(set(ids.tolist())) == len(ids)  # FNV(alt-loc, serial): distinct atoms, distinct ids


@pytest.mark.gpu
@pytest.mark.parametrize("name,opts,kw", OPTION_CASES)
def test_levels_under_reference_tested_options(tmp_path, name, opts, kw):
    """The same cases through the GPU: AtomLevel and ResidueLevel values equal the oracle's on the Python
    reader's selection."""
    path, opts, kw = _case(tmp_path, name, opts, kw)
    atom, res, meta = expected(name, vdw_fallback=True, path=path, **kw)
    p = subprocess.run([CLI, "atom", path, *opts], capture_output=True, text=True)
    assert p.returncode == 0, (p.stdout[:300], p.stderr[:300])
    got = np.array(json.loads(p.stdout)["Atom"], np.float32)
    assert np.array_equal(got, atom)
    p = subprocess.run([CLI, "residue", path, *opts], capture_output=True, text=True)
    assert p.returncode == 0, (p.stdout[:300], p.stderr[:300])
    got_res = json.loads(p.stdout)["Residue"]
    assert np.array_equal(np.array([g["value"] for g in got_res], np.float32), res)


def test_first_model_only_is_pinned(tmp_path):
    """A file with several MODELs: this reader keeps the FIRST model (documented in include/rustsasa_amd.hpp and
    DESIGN.md; pdbtbx, whose source is not in the reference tree, appears to iterate over every model's chains,
    which would overlay all models in one computation).  Pinned here so that a change is a decision."""
    src = open(sio.data_path("1jcd.pdb")).read().splitlines(keepends=True)
    body = [l for l in src if l.startswith(("ATOM", "HETATM", "TER"))]
    shifted = [l[:30] + f"{float(l[30:38]) + 50.0:8.3f}" + l[38:] if l.startswith(("ATOM", "HETATM")) else l for l in body]
    two = tmp_path / "two_models.pdb"
    two.write_text("MODEL        1\n" + "".join(body) + "ENDMDL\nMODEL        2\n" + "".join(shifted) + "ENDMDL\nEND\n")
    (x2, y2, z2, r2), ids2, d2 = _select(str(two))
    (x1, y1, z1, r1), ids1, d1 = _select(sio.data_path("1jcd.pdb"))
    assert np.array_equal(x1, x2) and np.array_equal(r1, r2) and d1["chain_end"] == d2["chain_end"]


def test_altloc_fixtures_meet_the_quality_gate_without_a_gpu():
    """tests/quality.rs:225 on the committed alt-loc fixtures through `select` + oracle (the whole set of 88:
    tools/check_quality_set.py in the build container, RMSE 43.997 - the reference's own 43.99)."""
    ours, theirs = [], []
    for pid in ALTLOC + ["4c1a"]:
        (x, y, z, r), ids, d = _select(sio.data_path(f"freesasa/{pid}.pdb"))
        atom = po.calculate_sasa_internal(x, y, z, r, ids, 1.4, 100, 8, threads=0)
        sums = po.residue_sums(atom, np.array([0] + d["chain_end"], np.uint32))
        got = dict(zip(d["chains"], (float(v) for v in sums)))
        ref = json.load(open(sio.data_path(f"freesasa/{pid}.json")))
        want = {c["label"]: c["area"]["total"] for rr in ref["results"] for s in rr["structure"] for c in s["chains"]}
        for k in sorted(set(want) & set(got)):
            ours.append(got[k])
            theirs.append(want[k])
    rmse = float(np.sqrt(np.mean((np.array(ours) - np.array(theirs)) ** 2)))
    assert len(ours) >= 7 and rmse <= RMSE_GATE, rmse


@pytest.mark.gpu
def test_process_files_with_nan_coordinates_in_one_file(tmp_path):
    """`nan` in a coordinate column parses to NaN (as a Rust `parse::<f64>()` would give): that atom is nobody's
    neighbour and keeps its whole sphere, the other atoms of the file and the other files of the batch do not notice
    (include/rustsasa_amd.h, "Non-finite input")."""
    src = open(sio.data_path("1jcd.pdb")).read().splitlines(keepends=True)
    k = [i for i, l in enumerate(src) if l.startswith("ATOM")][25]
    src[k] = src[k][:30] + "     nan" + src[k][38:]
    bad = tmp_path / "nan_atom.pdb"
    bad.write_text("".join(src))
    paths = [sio.data_path("151L_H3.pdb"), str(bad), sio.data_path("example.cif")]
    lst = str(tmp_path / "files.txt")
    open(lst, "w").write("\n".join(paths) + "\n")
    p = subprocess.run([CLI, "files", "residue", lst, "--full"], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[:500]
    got = json.loads(p.stdout)
    assert got["n_ok"] == 3
    for path, r in zip(paths, got["results"]):
        _, res, _ = expected(None, path=path)
        assert np.array_equal(np.array(r, np.float32), res), path
    atom, _, _ = expected(None, path=str(bad))
    clean, _, _ = expected("1jcd.pdb")
    assert np.sum(atom != clean) >= 1 and np.all(np.isfinite(atom))


def test_json_writer_prints_f32_as_serde_does():
    """sasa_result_to_json's numbers (io.rs:11-13 through serde_json / ryu): the shortest decimal that reads back as the
    same f32, plain notation with ".0" on whole numbers, a bare exponent outside [1e-5, 1e16), null for non-finite
    values.  (Round 5's writer printed 200.0 as 2e+02 and took 2.4 us per value; directory mode with per-file output
    prints 1.5 M of them per proteome.)"""
    rng = np.random.default_rng(5)
    vals = np.concatenate([rng.uniform(0, 400, 300), rng.integers(0, 500, 60).astype(np.float64), 10.0 ** rng.uniform(-12, 20, 80),
                           -rng.uniform(0, 50, 20), [0.0, 0.1, 200.0, 1e-5, 9.9999e-6, 1e16, 9.9e15, 16777216.0, 3.4028235e38, 1e-45]]
                          ).astype(np.float32)
    bits = [f"{b:08x}" for b in vals.view(np.uint32)] + ["7fc00000", "7f800000", "ff800000"]
    out = subprocess.run([CLI, "json-floats"] + bits, capture_output=True, text=True).stdout.strip()
    assert out.startswith('{"Atom":[') and out.endswith("]}")
    toks = out[len('{"Atom":['):-2].split(",")
    assert toks[-3:] == ["null", "null", "null"] and len(toks) == len(bits)
    for v, t in zip(vals, toks):
        assert np.float32(t) == v, (v, t)                                      # reads back as the same f32
        m, e = np.format_float_scientific(v, unique=True, trim="-").split("e")   # the shortest digits and their exponent
        if v == 0 or -5 <= int(e) < 16:  # (ryu: plain notation while the decimal point stays within the digits' reach)
            assert t == np.format_float_positional(v, unique=True, trim="0"), (v, t)   # shortest, plain, ".0" on whole numbers
        else:
            assert t == f"{m}e{int(e)}", (v, t)                                 # "1e-7", "1.5e20"
    assert [np.float32(x) for x in json.loads(out.replace("null", "0"))["Atom"][:3]] == [v for v in vals[:3]]


@pytest.mark.gpu
def test_directory_mode_end_to_end_writes_one_json_per_file(tmp_path):
    """The reference's directory mode end to end (src/main.rs:203-226,342-480, src/utils/io.rs:11-13): files in, one
    <stem>.json per input in the output directory, in serde's shape, with the values process_files returns; a file
    that cannot be read gets no output and does not disturb the others; PDB and mmCIF inputs side by side."""
    names = ["1jcd.pdb", "2drt.pdb", "151L_H3.pdb", "example.cif", "bad_seqadv_1A06.pdb"]
    paths = [sio.data_path(n) for n in names] + [str(tmp_path / "missing.pdb")]
    lst = tmp_path / "files.txt"
    lst.write_text("\n".join(paths) + "\n")
    out_dir = tmp_path / "out"
    out_dir.mkdir()
    p = subprocess.run([CLI, "files", "residue", str(lst), "--full", "--labels", "--out-dir", str(out_dir)], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[:400]
    got = json.loads(p.stdout)
    assert got["n_ok"] == len(names) and "error" in got["results"][-1]
    written = sorted(os.listdir(out_dir))
    assert written == sorted(n.rsplit(".", 1)[0] + ".json" for n in names)
    assert got["bytes_written"] == sum(os.path.getsize(out_dir / w) for w in written)
    for n, res in zip(names, got["results"]):
        text = (out_dir / (n.rsplit(".", 1)[0] + ".json")).read_text()
        assert text.startswith('{"Residue":[{"serial_number":') and text.endswith("]}")
        rows = json.loads(text)["Residue"]
        assert list(rows[0].keys()) == ["serial_number", "insertion_code", "value", "name", "is_polar", "chain_id"]
        assert len(rows) == len(res)
        assert [np.float32(r["value"]) for r in rows] == [np.float32(v) for _, v in res]   # the values of the call, bit for bit
        assert [r["chain_id"] for r in rows] == [c for c, _ in res]
    # the other levels write their own shapes
    for level, key in (("atom", "Atom"), ("chain", "Chain"), ("protein", "Protein")):
        d = tmp_path / level
        d.mkdir()
        p = subprocess.run([CLI, "files", level, str(lst), "--out-dir", str(d)], capture_output=True, text=True)
        assert p.returncode == 0 and sorted(os.listdir(d)) == written
        assert list(json.loads((d / "1jcd.json").read_text()).keys()) == [key]
