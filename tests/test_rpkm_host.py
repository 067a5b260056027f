"""CPU: the host side of `sam_rpkm --compute-rpkm` -- the constitutive parts of the gene model, the RPKM formula, the
per-gene rules over a given array of counts against the restatement in tests/_rpkm_ref.py, the command line without
--read-len, and no CPU path behind the device pass."""
import os
import types

import pytest

import _rpkm_case as case
import _rpkm_ref as ref
from miso_amd import capi, gene_utils, sam_rpkm, sam_utils


def test_get_const_parts_keeps_one_copy_per_transcript(tmp_path):
    """Three isoforms: the first and last exon are in all of them and come back once per transcript; the middle exon
    of the third has the same start and another end, so neither middle exon is constitutive."""
    gff = tmp_path / "g.gff"
    gff.write_text(case.gff_text())
    genes = gene_utils.load_genes_from_gff(str(gff), suppress_warnings=True)
    gene = genes["alt3"]["gene_object"]
    assert len(gene.isoforms) == 3 and len(gene.parts) == 9
    const = gene.get_const_parts()
    assert [(p.start, p.end) for p in const] == [(5000, 5100), (5700, 5800)] * 3
    assert len(set(id(p) for p in const)) == 6 and all(p in gene.parts for p in const)
    assert genes["noconst"]["gene_object"].get_const_parts() == []
    assert [(p.start, p.end) for p in genes["shared"]["gene_object"].get_const_parts()] == [(20000, 20500)] * 2
    # the checker's gene model agrees on every gene
    for (gid, _, transcripts) in ref.parse_genes(case.gff_text()):
        assert [(p.start, p.end) for p in genes[gid]["gene_object"].get_const_parts()] == ref.const_parts(transcripts)


def test_rpkm_per_region_by_hand():
    # 15 reads on (100 - 36 + 1) + (50 - 36 + 1) = 80 positions = 0.08 kb; 2 million reads: 187.5 / 2
    assert sam_rpkm.rpkm_per_region([100, 50], [10, 5], 36, 2000000) == 93.75
    # 7 / 0.065 / 0.123456: the reference's order of operations, in doubles
    assert sam_rpkm.rpkm_per_region([100], [7], 36, 123456) == (7.0 / (65 / 1e3)) / (123456 / 1e6)
    assert sam_rpkm.rpkm_per_region([36], [0], 36, 10) == 0.0
    # no read in the file: IEEE division, never an exception
    nan = sam_rpkm.rpkm_per_region([100], [0], 36, 0)
    inf = sam_rpkm.rpkm_per_region([100], [3], 36, 0)
    assert nan != nan and inf == float("inf")
    assert ("%.2f" % nan, "%.2f" % inf) == ("nan", "inf")
    assert isinstance(sam_rpkm.rpkm_per_region([100], [7], 36, 123456), float)


def test_rows_and_summary_from_given_counts(tmp_path, capsys):
    """gene_rpkms over brute-force counts: rows, the file and every printed line equal the checker's."""
    gff_text, sam_text = case.gff_text(), case.sam_text()
    gff = tmp_path / "g.gff"
    gff.write_text(gff_text)
    genes = gene_utils.load_genes_from_gff(str(gff), suppress_warnings=True)
    refs, recs = ref.parse_sam(sam_text)
    bamfile = types.SimpleNamespace(references=tuple(refs))
    seqids, starts, ends = sam_rpkm.const_part_intervals(genes, bamfile)
    # se2: 2 x 2 copies; alt3: 2 x 3 on "2"; small: 2 x 2; shared: 2; mixed: 2 x 2 -- nothing of the other three genes
    assert len(seqids) == 4 + 6 + 4 + 2 + 4 and set(seqids) == {"chr1", "2"}
    counts = ref.fetch_counts(sam_text, list(zip(seqids, starts, ends)))
    capsys.readouterr()
    rows, num_no_const, too_small = sam_rpkm.gene_rpkms(genes, bamfile, counts, case.READ_LEN, len(recs))
    printed = capsys.readouterr().out.splitlines()
    want_rows, want_text, want_lines = ref.compute(sam_text, gff_text, case.READ_LEN)
    assert rows == want_rows and printed == want_lines
    assert [r["gene_id"] for r in rows] == ["se2", "alt3", "shared", "mixed"]
    assert num_no_const == 1 and [g for g, _ in too_small] == ["small", "absent"]
    assert dict(too_small)["small"] > 0 and dict(too_small)["absent"] == 0
    assert "Skipping random chromosome gene: onrandom, chr5_random" in printed
    assert "Error fetching region: chr9:100-400" in printed
    assert "    * small\t%d" % dict(too_small)["small"] in printed
    # the rows are not of zeros, the shared exon is in its row once and the short exon of `mixed` not at all
    by_id = {r["gene_id"]: r for r in rows}
    assert all(float(r["rpkm"]) > 0 for r in rows)
    assert by_id["shared"]["const_exon_lens"] == "501" and by_id["mixed"]["const_exon_lens"] == "201"
    assert by_id["se2"]["const_exon_lens"] == "101,101" and by_id["alt3"]["const_exon_lens"] == "101,101"
    out = tmp_path / "t.rpkm"
    sam_rpkm.write_rpkms(rows, str(out))
    assert out.read_bytes() == want_text.encode()
    # a counts array of another length is an error, not a silent misalignment
    with pytest.raises(ValueError):
        sam_rpkm.gene_rpkms(genes, bamfile, list(counts) + [0], case.READ_LEN, len(recs))


def test_main_without_read_len(tmp_path, capsys):
    out = tmp_path / "out"
    rc = sam_rpkm.main(["--compute-rpkm", str(tmp_path / "g.gff"), str(tmp_path / "r.bam"), str(out)])
    assert rc == 1
    assert "Error: Must give --read-len to compute RPKMs." in capsys.readouterr().out
    assert not out.exists()


def test_count_total_reads_counts_every_record(tmp_path):
    sam = tmp_path / "r.sam"
    sam.write_text(case.sam_text())
    assert sam_rpkm.count_total_reads(str(sam)) == 3000 == len(ref.parse_sam(case.sam_text())[1])


def test_fetch_counts_has_no_cpu_path(tmp_path):
    if capi.device_count() > 0:
        pytest.skip("a GPU is present")
    sam = tmp_path / "r.sam"
    sam.write_text(case.sam_text(n_reads=50))
    f = sam_utils.Samfile(str(sam))
    with pytest.raises(capi.InternalError, match="no HIP device"):
        capi.fetch_counts(f, ["chr1"], [1000], [1100])
    assert b"no HIP device" in capi.lib().miso_last_error()
