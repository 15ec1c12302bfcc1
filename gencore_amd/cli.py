"""The gencore command line (src/main.cpp, src/options.cpp) over the HIP engine: `python -m gencore_amd -i in.bam -o out.bam -r ref.fa ...`.

Flags, defaults and validation messages are the reference's; the run is gce_run_bam_passes on one device (gce_run_bam_depth's single pass when
the file fits --device_memory, key-range passes otherwise) or gce_run_bam_depth's sharded runner for several --devices); afterwards the two
Stats summaries go to stderr and the JSON report is written (src/gencore.cpp:284-292, src/main.cpp:113-116).
Every check happens before the library is loaded, so a bad command line never touches a GPU."""
import argparse
import os
import re
import sys
import time

from . import __version__

EPILOG = """\
Flags marked [gencore_amd] are not the reference's; every other flag, default and validation message is gencore 0.17.2's.
--index (not the reference's) writes <output>.bai, the BAI index of the BAM output, built on the GPU.
--sort (not the reference's) takes a BAM in any order, as an aligner writes it: the GPU sorts it by coordinate into a temporary BAM first
(what `samtools sort` does in front of the reference), and the run reads that file.  --device_memory bounds the sort as it bounds the run: a
file that does not fit is sorted in output-range passes over the input.
--sort_sam (not the reference's) takes SAM text in any order, an aligner's output as it is: the GPU turns its lines into BAM records and sorts
them into the temporary BAM that --sort would make, without a BAM written in between.  In-core only, within --device_memory.
--calmd (not the reference's) makes NM and MD of the BAM output true: a consensus record takes its optional fields from one read of its cluster,
so its MD:Z describes that read and not the voted bases, and its NM is patched only where it was stored as type C.  After the output and the
report are written the GPU recomputes both against -r (what `samtools calmd` does behind the reference) and the result replaces the output.
The report is not changed by it.  --device_memory bounds it (and --calmd_in) as it bounds the run: the rewritten records are written while the file
is read, so neither the input nor the output has to fit the device (the reference bases do).
--calmd_in (not the reference's) recomputes NM and MD of the input BAM the same way first, into a temporary BAM: an input whose records lack NM
stops the run with GCE_ERR_NM_MISSING otherwise.
--umi_from (not the reference's) takes a file whose UMIs are not where the reference looks for them (the last `:`-field of an MI:Z value or of the
read name, of A C G T with at most one `_`): --umi_from RX reads them from the RX:Z tag that fgbio, DRAGEN and `bwa mem -C` pipelines write
(ACGT-TTGA for duplex), --umi_from name from an Illumina read name (...:ACGT+TTGA).  The GPU first writes a temporary BAM in which every such
record carries its UMI as MI:Z (upper case, - and + as _), which the run then reads as the reference reads MI:Z; records without the tag, or
whose value is not a UMI, are left as they are.  Without the flag such a file runs with every UMI empty: all reads of one position pair merge.
--pileup FILE and --pileup_in FILE (not the reference's) count bases per strand at every position of the -b targets on the GPU (what
`samtools mpileup` or `bam-readcount` are run for around a consensus step): --pileup_in over the input as the run reads it, --pileup over the
BAM output (after --calmd), so the two tables show which mismatches consensus removed.  A table is tab-separated: contig, 1-based pos, ref (from
-r), depth, then A C G T N DEL INS LOWQ of the forward and of the reverse strand; records with a flag bit of 0x704 (unmapped, secondary, QC
fail, duplicate) are left out, as are those below --pileup_min_mapq, and a base below --pileup_min_baseq goes to LOWQ.  Overlapping mates are
counted twice, there is no BAQ and no split by read group.  With --pileup_fragments (for coordinate-sorted files) both tables count every
fragment once where its mates overlap, as `samtools mpileup` does in outline: where the mates agree the first in the file is counted with the
sum of the two qualities (at most 200), where they differ the one of higher quality with 4 / 5 of its quality; a second line on STDERR gives
the pairs, the shared columns and those that disagree.
--error_profile FILE and --error_profile_in FILE (not the reference's) count, on the GPU, mismatches against -r by sequencing cycle (what `fgbio
ErrorRateByReadPosition`, Picard's artifact metrics or the mismatches-per-cycle block of `samtools stats` are run for): --error_profile_in over
the input as the run reads it, --error_profile over the BAM output (after --calmd), so the two tables show how far the error rate fell, by
substitution and by read position.  A table is tab-separated: segment (1 first, 2 last of the pair, 0 otherwise), cycle, bases, mismatches, the
sixteen counts A>A .. T>T of reference base against read base in read orientation (a reverse-strand read is complemented, so G>T stays apart
from C>A), then READ_N REF_OTHER LOWQ INS DEL; integers only, no rates.  Records with a flag bit of 0x704 are left out, as are those below
--error_profile_min_mapq, on a contig -r lacks or longer than 1024 bases; a base below --error_profile_min_baseq goes to LOWQ.  With -b only
events on the targets count.  Hard clips do not count into the cycle, there is no split by read group.  --error_profile_mask FILE (.vcf, .vcf.gz or .bed of known variant
sites) takes the events at those positions out of every class and counts them in a trailing MASKED column (one more line on STDERR gives the
mask's intervals, its bases and the events masked): without it the mismatches of a consensus output are the sample's genotype.
Overlapping mates are counted twice.  With --error_profile_fragments (for coordinate-sorted files) both tables count every fragment once
where its mates overlap, choosing the mate as --pileup_fragments does, and a second table, FILE.overlap.tsv, says what the two mates of a pair
show about each other at the positions both cover: segment, cycle, shared, errors, the sixteen A>A .. T>T (off the diagonal this mate's
sequencing error, its partner reading the reference base; on it the partner's), then AGREE_REF, AGREE_ALT (both read the same base that is
not the reference's: older than the sequencer, or a variant), DIFF_OTHER, UNUSABLE and LOWQ; a second line on STDERR gives the pairs, the
shared columns and those that disagree.
--error_profile_support FILE (not the reference's) answers how -s and --duplex_only should be set, from ONE run at -s 1: over the BAM output,
on the GPU, it tabulates the same classes not by cycle but by the support of each consensus record, the FR tag (forward-strand reads merged
into it) and the RR tag (reverse-strand reads; duplex records alone carry it).  A row: segment, forward, reverse (`.` for an absent tag, 1 ..
31, `32+`), records, bases, mismatches, the sixteen A>A .. T>T, READ_N REF_OTHER LOWQ INS DEL, and MASKED with --error_profile_mask; the
mismatches over the bases of the rows forward = 1, 2, 3, ... are the residual error a family of that size leaves, and the rows with a
reverse count against those with `.` are duplex against single-strand.  It honours -b, --error_profile_mask, --error_profile_min_mapq and
--error_profile_min_baseq; --error_profile_support_tags A,B reads two other integer tags (aD,bD: fgbio's duplex depths).  Every record is
counted (overlapping mates twice), there is no cycle column and no split by read group.
--error_profile_quality FILE and --error_profile_quality_in FILE (not the reference's) tabulate the same classes, on the GPU, by the base
quality the records report (what GATK's recalibration table or Picard QualityScoreDistribution beside the artifact metrics are run for): of
the bases at quality q, how many differ from -r.  --error_profile_quality_in reads the input as the run reads it, the sequencer's qualities;
--error_profile_quality the BAM output (after --calmd), the qualities the consensus step wrote itself, which a caller that weights by QUAL
trusts.  A row: segment, quality (the number, `94+` for a byte above 93, `.` for a record without qualities), bases, mismatches, the sixteen
A>A .. T>T, READ_N REF_OTHER LOWQ INS DEL, and MASKED with --error_profile_mask; an inserted base counts at its own quality, a deletion at
that of the base in front of it.  Both honour -b, --error_profile_mask, --error_profile_min_mapq and --error_profile_min_baseq (a base below
it is LOWQ in its own quality's row).  --error_profile_fragments does not apply to them: every record is counted (overlapping mates twice),
there is no cycle column and no split by read group.
--merge_overlap (not the reference's) resolves overlapping mates in the BAM output itself, on the GPU, so that whatever reads the file next
(a pileup-based caller, `bam-readcount`, a script that counts alleles) counts every fragment once without a tool of its own in between (`fgbio
ClipBam --clip-overlapping-reads`, `bamUtil clipOverlap`): mpileup's overlap tweak made durable.  At every reference column that both mates of
a pair cover with a base, where they agree the first in the file carries min(qa + qb, 93) and the other quality 0, where they differ the
better base keeps 4 / 5 of its quality and the other gets 0; a column where either quality is already 0 (or above 93) is left alone, so a
second run changes nothing.  Nothing but QUAL bytes changes: no soft clipping, so sizes, positions, CIGARs, NM / MD and the order stay.  It
runs after the output, the report, --calmd and the tables of --pileup and --error_profile* are written (they stay what they are without the
flag) and before --index, replaces the output through a temporary file beside it at --level, in-core within --device_memory, and prints the
pairs, the shared columns, those that disagree and the records changed on STDERR.  Records with a flag bit of 0x704 take no part; a name with
more than two candidate records is left alone.
-h is --html as in the reference, so help is --help only.  The HTML report is not written (--html is accepted with a notice), --debug is accepted
and does nothing.

Known difference: the reference writes its report before its destructor writes the records still held in its output set, so its
after_processing total_reads, total_bases, mismatches, coverage and coverage_bed leave that tail out.  This command reports every record it
writes.  The cluster, fragment, SSCS and DCS counters and the whole before_processing block are the same either way."""


class UsageError(Exception):
    pass


def build_parser():
    p = argparse.ArgumentParser(prog="python -m gencore_amd", add_help=False, epilog=EPILOG, formatter_class=argparse.RawDescriptionHelpFormatter,
                                description="Consensus reads from a coordinate-sorted BAM/SAM file (gencore on the MI355X).")
    a = p.add_argument
    # input/output
    a("-i", "--in", dest="input", default="-", help="input sorted bam/sam file. STDIN will be read from if it's not specified")
    a("-o", "--out", dest="output", default="-", help="output bam/sam file. STDOUT will be written to if it's not specified")
    a("-r", "--ref", required=True, help="reference fasta file name (should be an uncompressed .fa/.fasta file)")
    a("-b", "--bed", default="", help="bed file to specify the capturing region, none by default")
    a("-x", "--duplex_only", action="store_true",
      help="only output duplex consensus sequences, which means single stranded consensus sequences will be discarded.")
    a("--no_duplex", action="store_true", help="don't merge single stranded consensus sequences to duplex consensus sequences.")
    # UMI
    a("-u", "--umi_prefix", default="auto", help="the prefix for UMI, if it has. None by default. Check the README for the defails of UMI formats.")
    # thresholds
    a("-s", "--supporting_reads", type=int, default=1,
      help="only output consensus reads/pairs that merged by >= <supporting_reads> reads/pairs. The valud should be 1~10, and the default value is 1.")
    a("-a", "--ratio_threshold", type=float, default=0.8,
      help="if the ratio of the major base in a cluster is less than <ratio_threshold>, it will be further compared to the reference. "
           "The valud should be 0.5~1.0, and the default value is 0.8")
    a("-c", "--score_threshold", type=int, default=6,
      help="if the score of the major base in a cluster is less than <score_threshold>, it will be further compared to the reference. "
           "The valud should be 1~20, and the default value is 6")
    a("-d", "--umi_diff_threshold", type=int, default=1,
      help="if two reads with identical mapping position have UMI difference <= <umi_diff_threshold>, then they will be merged to generate a "
           "consensus read. Default value is 1.")
    a("-D", "--duplex_diff_threshold", type=int, default=2,
      help="if the forward consensus and reverse consensus sequences have <= <duplex_diff_threshold> mismatches, then they will be merged to "
           "generate a duplex consensus sequence, otherwise will be discarded. Default value is 2.")
    a("--high_qual", type=int, default=30, help="the threshold for a quality score to be considered as high quality. Default 30 means Q30.")
    a("--moderate_qual", type=int, default=20, help="the threshold for a quality score to be considered as moderate quality. Default 20 means Q20.")
    a("--low_qual", type=int, default=15, help="the threshold for a quality score to be considered as low quality. Default 15 means Q15.")
    a("--coverage_sampling", type=int, default=10000, help="the sampling rate for genome scale coverage statistics. Default 10000 means 1/10000.")
    # reporting
    a("-j", "--json", default="gencore.json", help="the json format report file name")
    a("-h", "--html", default=None, help="the html format report file name (accepted; the HTML report is not written)")
    # debugging
    a("--debug", action="store_true", help="output some debug information to STDERR. (accepted; does nothing)")
    a("--quit_after_contig", type=int, default=0,
      help="stop when <quit_after_contig> contigs are processed. Only used for fast debugging. Default 0 means no limitation.")
    a("--help", action="help", help="print this message")
    # not the reference's
    a("--devices", default="0", help="[gencore_amd] HIP device ordinals, comma separated: one runs one engine, several run the sharded runner "
                                     "(an ordinal may repeat). Default 0.")
    a("--device_memory", default="auto", help="[gencore_amd] device memory budget in GB (2^30 bytes) for one device, or auto (a fraction of the free "
                                               "memory): a file larger than the budget is processed in key-range passes, sorted (--sort) in output-range passes, and --calmd / --calmd_in "
                                               "keep to the budget by writing their output as they go. One device only. "
                                               "Default auto.")
    a("--threads", type=int, default=0, help="[gencore_amd] host threads for the file codecs; 0 = all cores. Default 0.")
    a("--index", action="store_true", help="[gencore_amd] after the output and the report are written, index the BAM output on the GPU into "
                                            "<output>.bai (BAI, SAMv1 5.2), on the first of --devices. Off by default.")
    a("--sort", action="store_true", help="[gencore_amd] the input BAM is not coordinate-sorted: sort it on the GPU first (on the first of --devices, into a "
                                           "temporary BAM beside the output that is removed afterwards), then run on the sorted file. Off by default.")
    a("--sort_sam", action="store_true", help="[gencore_amd] the input is SAM text that is not coordinate-sorted: parse and sort it on the GPU first (on the first of "
                                               "--devices, into a temporary BAM beside the output that is removed afterwards), then run on the sorted file. Off by default.")
    a("--calmd", action="store_true", help="[gencore_amd] after the output and the report are written (and before --index), recompute NM and MD of every record of "
                                            "the BAM output against -r on the GPU (on the first of --devices, at --level), through a temporary file beside "
                                            "the output that is renamed over it. It honours the --device_memory budget: an output beyond it is written as it is "
                                            "made. The report is not changed by it. Off by default.")
    a("--merge_overlap", action="store_true", help="[gencore_amd] after the output, the report, --calmd and the --pileup / --error_profile* tables are written (and before --index), "
                                                    "rewrite the base qualities of overlapping mates in the BAM output on the GPU so that a pileup of the file counts every fragment once: "
                                                    "where the mates agree the first carries the summed quality (at most 93) and the other 0, where they differ the better base keeps 4 / 5 "
                                                    "of its quality and the other gets 0. Only QUAL bytes change (no clipping). Needs a coordinate-sorted BAM output file; in-core within "
                                                    "--device_memory. Off by default.")
    a("--calmd_in", action="store_true", help="[gencore_amd] recompute NM and MD of the input BAM against -r on the GPU first (after --sort / --sort_sam; on the first of --devices, "
                                               "into a temporary BAM beside the output that is removed afterwards), then run on that file: an input without NM "
                                               "becomes runnable. It honours the --device_memory budget as --calmd does. Off by default.")
    a("--umi_from", default=None, metavar="TAG|name",
      help="[gencore_amd] where the UMIs are: a two-character tag whose Z value holds them (RX), or name for the last `:`-field of an Illumina read "
           "name (ACGT+TTGA). The GPU first copies them into MI:Z fields (after --sort / --sort_sam and --calmd_in; on the first of --devices, into a "
           "temporary BAM beside the output that is removed afterwards, within --device_memory), then runs on that file. Off by default.")
    a("--pileup", default=None, metavar="FILE",
      help="[gencore_amd] after the output is written (and after --calmd), count bases per strand at every position of the -b targets over the BAM output on the "
           "GPU (on the first of --devices, within --device_memory) and write the table to FILE, with ref from -r. Off by default.")
    a("--pileup_in", default=None, metavar="FILE",
      help="[gencore_amd] the same table over the input as the run reads it (after --sort / --sort_sam, --calmd_in and --umi_from), written to FILE before the run. "
           "Off by default.")
    a("--pileup_fragments", action="store_true",
      help="[gencore_amd] --pileup / --pileup_in count each fragment once where its mates overlap (the file must be coordinate-sorted). Off by default.")
    a("--pileup_min_mapq", type=int, default=0, help="[gencore_amd] --pileup / --pileup_in leave out records whose mapping quality is below this (0..255). Default 0.")
    a("--pileup_min_baseq", type=int, default=0, help="[gencore_amd] --pileup / --pileup_in count a base whose quality is below this (0..255) as LOWQ. Default 0.")
    a("--error_profile", default=None, metavar="FILE",
      help="[gencore_amd] after the output is written (after --calmd, before --index), count mismatches against -r by sequencing cycle and substitution over the BAM "
           "output on the GPU (on the first of --devices, within --device_memory) and write the table to FILE. Restricted to the -b targets when -b is given. Off by default.")
    a("--error_profile_in", default=None, metavar="FILE",
      help="[gencore_amd] the same table over the input as the run reads it (after --sort / --sort_sam, --calmd_in and --umi_from), written to FILE before the run. "
           "Restricted to the -b targets when -b is given. Off by default.")
    a("--error_profile_min_mapq", type=int, default=0,
      help="[gencore_amd] --error_profile / --error_profile_in leave out records whose mapping quality is below this (0..255). Default 0.")
    a("--error_profile_min_baseq", type=int, default=0,
      help="[gencore_amd] --error_profile / --error_profile_in count a base whose quality is below this (0..255) as LOWQ. Default 0.")
    a("--error_profile_mask", default=None, metavar="FILE",
      help="[gencore_amd] --error_profile / --error_profile_in take the known variant sites of FILE (.vcf, .vcf.gz or .bed) out of every class: an event at a masked position "
           "is counted in a trailing MASKED column instead, so that the mismatches are errors, not the sample's genotype. Applies to both tables and to --error_profile_fragments.")
    a("--error_profile_fragments", action="store_true",
      help="[gencore_amd] --error_profile / --error_profile_in count each fragment once where its mates overlap (the file must be coordinate-sorted) and write the mates' "
           "agreement by cycle to FILE.overlap.tsv beside each. Off by default.")
    a("--error_profile_support", default=None, metavar="FILE",
      help="[gencore_amd] after the output is written (after --calmd, beside --error_profile, before --index), count mismatches against -r over the BAM output by the support of "
           "each consensus record -- its FR tag (forward-strand reads) and its RR tag (reverse-strand reads, on duplex records) -- on the GPU (on the first of --devices, within "
           "--device_memory) and write the table to FILE: for choosing -s and --duplex_only from one run at -s 1. Honours -b, --error_profile_mask, --error_profile_min_mapq and "
           "--error_profile_min_baseq. Off by default.")
    a("--error_profile_support_tags", default="FR,RR", metavar="A,B",
      help="[gencore_amd] --error_profile_support reads the forward count from tag A and the reverse count from tag B, two two-character tags of an integer type "
           "(aD,bD: fgbio's duplex depths). Default FR,RR.")
    a("--error_profile_quality", default=None, metavar="FILE",
      help="[gencore_amd] after the output is written (after --calmd, beside --error_profile, before --index), count mismatches against -r over the BAM output by the base "
           "quality each record reports -- the qualities the consensus step wrote -- on the GPU (on the first of --devices, within --device_memory) and write the table to FILE: "
           "one row per (segment, quality). Honours -b, --error_profile_mask, --error_profile_min_mapq and --error_profile_min_baseq; --error_profile_fragments does not apply "
           "to it. Off by default.")
    a("--error_profile_quality_in", default=None, metavar="FILE",
      help="[gencore_amd] the same table over the input as the run reads it (after --sort / --sort_sam, --calmd_in and --umi_from), the sequencer's qualities, written to FILE "
           "before the run. --error_profile_fragments does not apply to it. Off by default.")
    a("--level", type=int, default=6, help="[gencore_amd] BGZF compression level of a BAM output: 0..9 (zlib), -1 (fixed Huffman on the host), "
                                           "-2 (fixed Huffman on the GPU), -3 (the smallest of dynamic Huffman, fixed Huffman and stored per block, on the GPU). "
                                           "With an output name that ends in sam, -2 and -3 make the GPU write the SAM text; every other level leaves it to the host. Default 6.")
    return p


def check_file_valid(path):
    """util.h:169-178"""
    if not os.path.exists(path):
        raise UsageError("ERROR: file '%s' doesn't exist, quit now" % path)
    if os.path.isdir(path):
        raise UsageError("ERROR: '%s' is a folder, not a file, quit now" % path)


def validate(o):
    """main.cpp:96-98, then Options::validate (options.cpp:42-111) in its order, then the BED file (bed.cpp:112-116) and this command's own checks."""
    def err(msg):
        raise UsageError("ERROR: " + msg)
    if o.duplex_only and o.no_duplex:
        err("You cannot enable both duplex_only and no_duplex")
    if not o.input:
        err("input should be specified by --in1")
    if o.sort and o.input == "-":
        err("--sort needs an input file, not STDIN")
    if o.sort_sam and not o.sort and o.input == "-":
        err("--sort_sam needs an input file, not STDIN")
    if o.calmd_in and o.input == "-":
        err("--calmd_in needs an input file, not STDIN")
    if o.pileup_in is not None and o.input == "-":
        err("--pileup_in needs an input file, not STDIN")
    if o.error_profile_in is not None and o.input == "-":
        err("--error_profile_in needs an input file, not STDIN")
    if o.error_profile_quality_in is not None and o.input == "-":
        err("--error_profile_quality_in needs an input file, not STDIN")
    if o.umi_from is not None:
        u = o.umi_from
        if u != "name" and not (len(u) == 2 and u.isascii() and u[0].isalpha() and u[1].isalnum()):
            err("--umi_from should be a two-character tag such as RX, or name, got '%s'" % u)
        if u == "MI":
            err("--umi_from MI is what the run reads without the flag")
        if o.input == "-":
            err("--umi_from needs an input file, not STDIN")
        if o.umi_prefix != "auto":
            err("--umi_from cannot be combined with --umi_prefix")
    check_file_valid(o.input)
    if o.umi_from is not None and not o.sort_sam:
        with open(o.input, "rb") as f:
            if f.read(2) != b"\x1f\x8b":
                err("--umi_from needs BAM input, not SAM text")
    if o.calmd_in and not o.sort_sam:
        with open(o.input, "rb") as f:
            if f.read(2) != b"\x1f\x8b":
                err("--calmd_in needs BAM input, not SAM text")
    if o.sort:
        with open(o.input, "rb") as f:
            if f.read(2) != b"\x1f\x8b":
                err("--sort needs BAM input, not SAM text")
    if o.sort and o.sort_sam:
        err("--sort and --sort_sam cannot be combined")
    if o.sort_sam:
        with open(o.input, "rb") as f:
            if f.read(2) == b"\x1f\x8b":
                err("--sort_sam needs SAM text input, not BAM")
    if o.ref.endswith(".gz"):
        raise UsageError("reference fasta file should not be compressed.\nplease unzip %s and try again." % o.ref)
    checks = [
        (o.ratio_threshold > 1.0, "ratio_threshold cannot be greater than 1.0"), (o.ratio_threshold < 0.5, "ratio_threshold cannot be less than 0.5"),
        (o.supporting_reads > 10, "supporting_reads cannot be greater than 10"), (o.supporting_reads < 1, "supporting_reads cannot be less than 1"),
        (o.score_threshold > 10, "score_threshold cannot be greater than 10"), (o.score_threshold < 1, "score_threshold cannot be less than 1"),
        (o.high_qual > 40, "high_qual cannot be greater than 40"), (o.high_qual < 20, "high_qual cannot be less than 20"),
        (o.moderate_qual > 35, "moderate_qual cannot be greater than 35"), (o.moderate_qual < 15, "moderate_qual cannot be less than 15"),
        (o.low_qual > 30, "low_qual cannot be greater than 30"), (o.low_qual < 8, "low_qual cannot be less than 8"),
        (o.umi_diff_threshold > 10, "umi_diff_threshold cannot be greater than 10"), (o.umi_diff_threshold < 0, "umi_diff_threshold cannot be negative"),
        (o.low_qual > o.moderate_qual, "low_qual cannot be greater than moderate_qual"),
        (o.moderate_qual > o.high_qual, "moderate_qual cannot be greater than high_qual"),
        (o.duplex_diff_threshold > 10, "duplex_diff_threshold cannot be greater than 10, suggest 2."),
        (o.duplex_diff_threshold < 0, "duplex_diff_threshold cannot be less than 0, suggest 2."),
    ]
    for bad, msg in checks:
        if bad:
            err(msg)
    if o.bed:
        check_file_valid(o.bed)
    if o.coverage_sampling <= 0:                    # the reference divides by it (stats.cpp:43)
        err("coverage_sampling should be greater than 0")
    if len(o.umi_prefix.encode()) > 31:
        err("umi_prefix cannot be longer than 31 characters")
    try:
        devices = [int(x) for x in o.devices.split(",")]
    except ValueError:
        devices = []
    if not devices or min(devices) < 0:
        err("devices should be a comma separated list of HIP device ordinals, got '%s'" % o.devices)
    if not (-3 <= o.level <= 9):
        err("level should be -3, -2, -1 or 0..9")
    o.device_memory_bytes = 0                       # 0: auto
    if o.device_memory != "auto":
        try:
            gb = float(o.device_memory)
        except ValueError:
            gb = float("nan")
        if not gb > 0 or gb == float("inf"):
            err("device_memory should be a positive number of GB or auto, got '%s'" % o.device_memory)
        if len(devices) > 1:
            err("device_memory works on one device; it cannot be combined with several --devices")
        o.device_memory_bytes = max(1, int(gb * (1 << 30)))
    if o.index and o.output == "-":
        err("--index needs an output file, not STDOUT")
    if o.index and o.output.endswith("sam"):
        err("--index needs BAM output, not SAM text")
    if o.calmd and o.output == "-":
        err("--calmd needs an output file, not STDOUT")
    if o.calmd and o.output.endswith("sam"):
        err("--calmd needs BAM output, not SAM text")
    if o.merge_overlap and o.output == "-":
        err("--merge_overlap needs an output file, not STDOUT")
    if o.merge_overlap and o.output.endswith("sam"):
        err("--merge_overlap needs BAM output, not SAM text")
    for flag, given in (("--pileup", o.pileup), ("--pileup_in", o.pileup_in)):
        if given is not None and not o.bed:
            err("%s needs the targets of -b" % flag)
    if o.pileup_fragments and o.pileup is None and o.pileup_in is None:
        err("--pileup_fragments needs --pileup or --pileup_in")
    if o.pileup is not None and o.output == "-":
        err("--pileup needs an output file, not STDOUT")
    if o.pileup is not None and o.output.endswith("sam"):
        err("--pileup needs BAM output, not SAM text")
    if o.pileup_in is not None and not o.sort_sam:
        with open(o.input, "rb") as f:
            if f.read(2) != b"\x1f\x8b":
                err("--pileup_in needs BAM input, not SAM text")
    for name in ("pileup_min_mapq", "pileup_min_baseq"):
        if not (0 <= getattr(o, name) <= 255):
            err("%s should be 0..255" % name)
    if o.error_profile is not None and o.output == "-":
        err("--error_profile needs an output file, not STDOUT")
    if o.error_profile is not None and o.output.endswith("sam"):
        err("--error_profile needs BAM output, not SAM text")
    if o.error_profile_in is not None and not o.sort_sam:
        with open(o.input, "rb") as f:
            if f.read(2) != b"\x1f\x8b":
                err("--error_profile_in needs BAM input, not SAM text")
    if o.error_profile_fragments and o.error_profile is None and o.error_profile_in is None:
        err("--error_profile_fragments needs --error_profile or --error_profile_in")
    if o.error_profile_support is not None:
        if o.output == "-":
            err("--error_profile_support needs an output file, not STDOUT")
        if o.output.endswith("sam"):
            err("--error_profile_support needs BAM output, not SAM text")
    if not re.fullmatch(r"[A-Za-z][A-Za-z0-9],[A-Za-z][A-Za-z0-9]", o.error_profile_support_tags):
        err("--error_profile_support_tags needs two two-character tags, as in FR,RR")
    if o.error_profile_support_tags != "FR,RR" and o.error_profile_support is None:
        err("--error_profile_support_tags needs --error_profile_support")
    if o.error_profile_quality is not None:
        if o.output == "-":
            err("--error_profile_quality needs an output file, not STDOUT")
        if o.output.endswith("sam"):
            err("--error_profile_quality needs BAM output, not SAM text")
    if o.error_profile_quality_in is not None and not o.sort_sam:
        with open(o.input, "rb") as f:
            if f.read(2) != b"\x1f\x8b":
                err("--error_profile_quality_in needs BAM input, not SAM text")
    if o.error_profile_mask is not None:
        if o.error_profile is None and o.error_profile_in is None and o.error_profile_support is None and o.error_profile_quality is None and o.error_profile_quality_in is None:
            err("--error_profile_mask needs --error_profile or --error_profile_in")
        check_file_valid(o.error_profile_mask)
        if not o.error_profile_mask.endswith((".vcf", ".vcf.gz", ".bed")):
            err("--error_profile_mask needs a .vcf, .vcf.gz or .bed file")
    for name in ("error_profile_min_mapq", "error_profile_min_baseq"):
        if not (0 <= getattr(o, name) <= 255):
            err("%s should be 0..255" % name)
    return devices


def params_of(o):
    from .capi import default_params
    return default_params(cluster_size_req=o.supporting_reads, score_percent_req=o.ratio_threshold, base_score_req=o.score_threshold,
                          proper_umi_diff_threshold=o.umi_diff_threshold, duplex_mismatch_threshold=o.duplex_diff_threshold,
                          high_quality=o.high_qual, moderate_quality=o.moderate_qual, low_quality=o.low_qual,
                          duplex_only=int(o.duplex_only), disable_duplex=int(o.no_duplex), max_contig=o.quit_after_contig,
                          umi_prefix="" if o.umi_from is not None else o.umi_prefix)    # (--umi_from: the MI:Z the pass wrote; auto would look at names)


def main(argv=None):
    argv = sys.argv[1:] if argv is None else list(argv)
    o = build_parser().parse_args(argv)
    try:
        devices = validate(o)
    except UsageError as e:
        print(str(e), file=sys.stderr)
        return 255
    t1 = int(time.time())
    command = "".join(a + " " for a in ["gencore"] + argv)           # main.cpp:101-104
    if o.html is not None:
        print("NOTE: gencore_amd does not write the HTML report; --html %s is ignored" % o.html, file=sys.stderr)
    from .bamio import calmd_bam_stream, error_profile_bam, error_profile_fragments_bam, index_bam, load_bed, pileup_bam, pileup_fragments_bam, run_bam_depth, run_bam_passes, sort_bam_passes, sort_sam, umi_to_mi
    from .capi import GceError
    from .report import read_header, summary, write_json
    sorted_tmp = calmd_tmp = umi_tmp = out_tmp = merge_tmp = None

    def pileup(label, bam, tsv):
        r = (pileup_fragments_bam if o.pileup_fragments else pileup_bam)(bam, o.bed, fasta=o.ref, tsv=tsv, device=devices[0], threads=o.threads, min_mapq=o.pileup_min_mapq,
                                                                         min_baseq=o.pileup_min_baseq, exclude_flags=0x704, device_budget_bytes=o.device_memory_bytes)
        sys.stderr.write("%s: %d records, %d eligible, %d sites\n" % (label, r.n_records, r.n_eligible, r.n_sites))
        if o.pileup_fragments:
            sys.stderr.write("%s: %d pairs, %d shared columns, %d disagreeing\n" % (label, r.n_pairs, r.n_shared_columns, r.n_disagree_columns))

    def error_profile(label, bam, tsv):
        kw = dict(bed=o.bed or None, tsv=tsv, device=devices[0], threads=o.threads, min_mapq=o.error_profile_min_mapq, min_baseq=o.error_profile_min_baseq, exclude_flags=0x704,
                  device_budget_bytes=o.device_memory_bytes)
        if o.error_profile_mask is not None:
            from .bamio import error_profile_fragments_masked_bam, error_profile_masked_bam
            r = (error_profile_fragments_masked_bam(bam, o.ref, o.error_profile_mask, overlap_tsv=tsv + ".overlap.tsv", **kw) if o.error_profile_fragments
                 else error_profile_masked_bam(bam, o.ref, o.error_profile_mask, **kw))
        else:
            r = error_profile_fragments_bam(bam, o.ref, overlap_tsv=tsv + ".overlap.tsv", **kw) if o.error_profile_fragments else error_profile_bam(bam, o.ref, **kw)
        sys.stderr.write("%s: %d records, %d eligible, %d bases, %d mismatches\n" % (label, r.n_records, r.n_eligible, r.n_bases, r.n_mismatches))
        if o.error_profile_fragments:
            sys.stderr.write("%s: %d pairs, %d shared columns, %d disagreeing\n" % (label, r.n_pairs, r.n_shared_columns, r.n_disagree_columns))
        if o.error_profile_mask is not None:
            sys.stderr.write("%s: mask %d intervals, %d bases, %d events masked\n" % (label, r.n_mask_intervals, r.n_masked_bases, r.n_masked_events))

    def error_profile_quality(label, bam, tsv):
        from .bamio import error_profile_quality_bam
        r = error_profile_quality_bam(bam, o.ref, mask=o.error_profile_mask, bed=o.bed or None, tsv=tsv, device=devices[0], threads=o.threads, min_mapq=o.error_profile_min_mapq,
                                      min_baseq=o.error_profile_min_baseq, exclude_flags=0x704, device_budget_bytes=o.device_memory_bytes)
        sys.stderr.write("%s: %d records, %d eligible, %d bases, %d mismatches, %d qualities\n"
                         % (label, r.n_records, r.n_eligible, r.n_bases, r.n_mismatches, int((r.counts[:, :, :22].sum(axis=(0, 2)) != 0).sum())))
        if o.error_profile_mask is not None:
            sys.stderr.write("%s: mask %d intervals, %d bases, %d events masked\n" % (label, r.n_mask_intervals, r.n_masked_bases, r.n_masked_events))
    tmp_dir = None if o.output == "-" else os.path.dirname(os.path.abspath(o.output))
    try:
        if o.sort or o.sort_sam:                                            # the runners below read the sorted temporary file, unchanged
            import tempfile
            fd, sorted_tmp = tempfile.mkstemp(suffix=".bam", prefix="gencore_sort_", dir=None if o.output == "-" else (os.path.dirname(os.path.abspath(o.output))))
            os.close(fd)
            sorter = sort_bam_passes if o.sort else sort_sam               # (--sort_sam: the same file, made from text; in-core only)
            sorter(o.input, sorted_tmp, device=devices[0], threads=o.threads, level=-2, device_budget_bytes=o.device_memory_bytes)
            o.input = sorted_tmp
        if o.calmd_in:                                                      # as --sort: the runners read the temporary file
            import tempfile
            fd, calmd_tmp = tempfile.mkstemp(suffix=".bam", prefix="gencore_calmd_", dir=tmp_dir)
            os.close(fd)
            calmd_bam_stream(o.input, calmd_tmp, o.ref, device=devices[0], threads=o.threads, level=-2, device_budget_bytes=o.device_memory_bytes)
            o.input = calmd_tmp
        if o.umi_from is not None:                                          # as --sort: the runners read the temporary file
            import tempfile
            fd, umi_tmp = tempfile.mkstemp(suffix=".bam", prefix="gencore_umi_", dir=tmp_dir)
            os.close(fd)
            r = umi_to_mi(o.input, umi_tmp, o.umi_from, device=devices[0], threads=o.threads, level=-2, device_budget_bytes=o.device_memory_bytes)
            sys.stderr.write("umi: %d records, MI written in %d, no source in %d, not a UMI in %d\n" % (r.n_records, r.n_tagged, r.n_no_source, r.n_not_umi))
            o.input = umi_tmp
        if o.pileup_in is not None:
            pileup("pileup_in", o.input, o.pileup_in)
        if o.error_profile_in is not None:
            error_profile("error_profile_in", o.input, o.error_profile_in)
        if o.error_profile_quality_in is not None:
            error_profile_quality("error_profile_quality_in", o.input, o.error_profile_quality_in)
        names, _ = read_header(o.input)
        region_names = [r[3] for r in load_bed(o.bed, names)] if o.bed else None
        out = "/dev/stdout" if o.output == "-" else o.output              # the runner only ever appends to its output: a pipe works
        if len(devices) == 1:                                               # passes when the file does not fit the budget (one pass: gce_run_bam_depth)
            _, depth, _ = run_bam_passes(o.input, out, params_of(o), devices[0], o.coverage_sampling, bed=o.bed or None, fasta=o.ref or None,
                                         threads=o.threads, level=o.level, device_budget_bytes=o.device_memory_bytes)
        else:
            _, depth = run_bam_depth(o.input, out, params_of(o), devices, o.coverage_sampling, bed=o.bed or None, fasta=o.ref or None,
                                     threads=o.threads, level=o.level)
        sys.stderr.write("----Before gencore processing:\n" + summary(depth["pre"], False) +
                         "\n----After gencore processing:\n" + summary(depth["post"], True))
        sys.stderr.flush()
        write_json(o.json, depth, names, o.coverage_sampling, command, region_names=region_names, has_bed=bool(o.bed))
        if o.calmd:
            out_tmp = o.output + ".calmd%d" % os.getpid()
            r = calmd_bam_stream(o.output, out_tmp, o.ref, device=devices[0], threads=o.threads, level=o.level, device_budget_bytes=o.device_memory_bytes)
            os.replace(out_tmp, o.output)
            sys.stderr.write("calmd: %d records rewritten, NM changed in %d, MD changed in %d\n" % (r.n_rewritten, r.n_nm_changed, r.n_md_changed))
        if o.pileup is not None:
            pileup("pileup", o.output, o.pileup)
        if o.error_profile is not None:
            error_profile("error_profile", o.output, o.error_profile)
        if o.error_profile_support is not None:
            from .bamio import error_profile_support_bam
            ft, rt = o.error_profile_support_tags.split(",")
            r = error_profile_support_bam(o.output, o.ref, mask=o.error_profile_mask, bed=o.bed or None, tsv=o.error_profile_support, tags=(ft, rt), device=devices[0], threads=o.threads,
                                          min_mapq=o.error_profile_min_mapq, min_baseq=o.error_profile_min_baseq, exclude_flags=0x704, device_budget_bytes=o.device_memory_bytes)
            sys.stderr.write("error_profile_support: %d records, %d eligible, %d bases, %d mismatches, %d with %s, %d with %s\n"
                             % (r.n_records, r.n_eligible, r.n_bases, r.n_mismatches, r.n_with_forward, ft, r.n_with_reverse, rt))
            if o.error_profile_mask is not None:
                sys.stderr.write("error_profile_support: mask %d intervals, %d bases, %d events masked\n" % (r.n_mask_intervals, r.n_masked_bases, r.n_masked_events))
        if o.error_profile_quality is not None:
            error_profile_quality("error_profile_quality", o.output, o.error_profile_quality)
        if o.merge_overlap:                                                 # (behind every output-side table: they stay what they are without the flag)
            from .bamio import merge_overlap_bam
            merge_tmp = o.output + ".overlap%d" % os.getpid()
            r = merge_overlap_bam(o.output, merge_tmp, device=devices[0], threads=o.threads, level=o.level, device_budget_bytes=o.device_memory_bytes)
            os.replace(merge_tmp, o.output)
            sys.stderr.write("merge_overlap: %d pairs, %d shared columns, %d disagreeing, %d records changed\n" % (r.n_pairs, r.n_shared_columns, r.n_disagree_columns, r.n_records_changed))
        if o.index:
            index_bam(o.output, o.output + ".bai", device=devices[0], threads=o.threads)
    except (GceError, OSError) as e:
        hint = "; --calmd_in recomputes the input's NM (and MD) against -r on the GPU first" if getattr(e, "status", 0) == -12 and not o.calmd_in else ""
        print("ERROR: %s%s" % (e, hint), file=sys.stderr)
        return 255
    finally:
        for tmp in (sorted_tmp, calmd_tmp, umi_tmp, out_tmp, merge_tmp):
            if tmp is not None and os.path.exists(tmp):
                os.remove(tmp)
    t2 = int(time.time())
    sys.stderr.write("\n%s\ngencore_amd v%s, time used: %d seconds\n" % (command, __version__, t2 - t1))
    return 0
