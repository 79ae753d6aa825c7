"""`python -m panfeed_amd`: the `panfeed` command (the reference's `panfeed/__main__.py`) on one GPU, or with `--gpus N`
on N of them.

Option names, short forms, defaults and meanings are the reference's (`__main__.py:86-222`); so are the refusals, their
order and their exit status (`__main__.py:234-242`, `input.py:213-216`).  The run itself is `pipeline.run_files`: the
native reader, the GPU, a writer thread.  Options added: `--device` (as the downstream tools have),
`--batch-clusters`, `--gpu-compress` and, for `--multiple-files`, `--gpu-compress-clusters`, with `--gpu-compress-level`
for the encoder's effort behind either.  `--cores` and `-ql/--queue-limit` are accepted and change nothing (the GPU takes the place of the
worker processes).  One refusal is new: `-k` outside 1..PF_MAX_K, before any file is read or the GPU touched.

Unlike the reference, no `<output>/fastas/` directory is made (the reader splits the GFFs' `##FASTA` sections in
memory), so none is left behind.

`--gpus N` (N > 1) is `sharded.run_files_sharded` with one rank per GPU: this process touches no GPU and starts the ranks
as fresh child processes (`rank.launch`).  With `WORLD_SIZE` and `RANK` in the environment -- a launcher of the user's
own -- the command is one rank of that world.  `PANFEED_SHARED_GPU=1` rehearses the control flow on one GPU.
"""
import argparse
import logging
import os
import sys

from . import __version__

logger = logging.getLogger("panfeed")

PF_MAX_K = 126          # include/panfeed_hip.h: 2 bits per base in at most four 63-bit key words
BATCH_CLUSTERS = 256    # pipeline.run_files' default


def get_options(argv=None):
    p = argparse.ArgumentParser(
        prog="panfeed",
        description="Gene-cluster-specific k-mers and their presence/absence patterns over a pangenome, on one AMD GPU, or "
                    "with --gpus N on N of them (the files are the same).  Under a launcher such as torchrun, which sets "
                    "WORLD_SIZE and RANK, the command is one rank of that world.  PANFEED_SHARED_GPU=1 runs every rank on "
                    "--device with host collectives: a rehearsal that exercises control flow only, never a multi-GPU "
                    "measurement.")
    p.add_argument("-g", "--gff", required=True,
                   help="GFF files: a directory of them, or a file naming one path per line (the sequences come from "
                        "each GFF's ##FASTA section unless -f is given; file names must match the table's strain columns)")
    p.add_argument("-p", "--presence-absence", required=True,
                   help="panaroo's gene_presence_absence.csv")
    p.add_argument("--targets", default=None,
                   help="strains whose k-mer positions go to kmers.tsv, one name per line (default: none)")
    p.add_argument("--genes", default=None,
                   help="gene clusters to work on, one name per line (default: every cluster of the table)")
    p.add_argument("-o", "--output", default="panfeed",
                   help="output directory; it must not exist yet (default: %(default)s)")
    p.add_argument("-f", "--fasta", default=None,
                   help="nucleotide FASTA files (.fasta / .fna): a directory of them, or a file naming one path per line")
    p.add_argument("-k", "--kmer-length", type=int, default=31,
                   help=f"k-mer length, 1..{PF_MAX_K} (default: %(default)d)")
    p.add_argument("--maf", type=float, default=0.01,
                   help="minor allele frequency: patterns rarer than this, or commoner than 1 - maf, are left out of "
                        "the pattern files (kmers.tsv keeps them; default: %(default).2f)")
    p.add_argument("--upstream", type=int, default=0,
                   help="bases added before each gene (default: %(default)d)")
    p.add_argument("--downstream", type=int, default=0,
                   help="bases added after each gene (default: %(default)d)")
    p.add_argument("--downstream-start-codon", action="store_true", default=False,
                   help="count --downstream from the start codon instead of the stop codon")
    p.add_argument("--non-canonical", action="store_true", default=False,
                   help="keep k-mers as read instead of their canonical form")
    p.add_argument("--no-filter", action="store_true", default=False,
                   help="keep k-mers whose pattern is the gene cluster's own presence/absence pattern")
    p.add_argument("--consider-missing", action="store_true", default=False,
                   help="leave a pattern's entry empty (NaN) for strains without the gene, instead of 0")
    p.add_argument("--multiple-files", action="store_true", default=False,
                   help="one output directory per gene cluster instead of one set of files")
    p.add_argument("--compress", action="store_true", default=False,
                   help="gzip the output files")
    p.add_argument("--gpu-compress", action="store_true", default=False,
                   help="gzip the output files on the GPU; implies --compress; much faster, somewhat larger files")
    p.add_argument("--bgzf", action="store_true", default=False,
                   help="with --gpu-compress: write the three files as BGZF, the multi-member gzip that bgzip and htslib "
                        "read and write (not with --multiple-files or on several GPUs)")
    p.add_argument("--gpu-compress-clusters", action="store_true", default=False,
                   help="with --multiple-files: gzip the per-cluster files on the GPU; implies --compress")
    p.add_argument("--gpu-compress-level", type=int, choices=(1, 2), default=None,
                   help="with --gpu-compress or --gpu-compress-clusters: the effort of the GPU's encoder (default: 1); 2 looks "
                        "for each position's match in the row before as well and parses lazily -- smaller files, "
                        "hashes_to_patterns.tsv most of all, for more encoder time; also under --bgzf and --gpus N")
    p.add_argument("--passing-hashes", metavar="FILE", default=None,
                   help="write only the kmers.tsv rows of passing patterns: those whose (cluster, k-mer) kmers_to_hashes.tsv "
                        "lists with one of the hashed_pattern values of FILE (one per line); decided on the GPU before a "
                        "dropped row is written; the other two files are not affected (not on several GPUs)")
    p.add_argument("--passing-associations", metavar="FILE", default=None,
                   help="the same, with the passing hashes taken from an associations table as panfeed-get-kmers takes "
                        "them: the rows whose --passing-column is at most --passing-threshold")
    p.add_argument("--passing-threshold", type=float, default=None,
                   help="with --passing-associations (default: 1)")
    p.add_argument("--passing-column", default=None,
                   help="with --passing-associations (default: lrt-pvalue)")
    p.add_argument("--cores", type=int, default=1,
                   help="accepted for compatibility; the GPU does the work of the worker processes")
    p.add_argument("-ql", "--queue-limit", type=int, default=3,
                   help="accepted for compatibility; has no effect here")
    p.add_argument("--stop-on-missing", action="store_true", default=False,
                   help="fail when a strain, contig or gene of the table is not found (default: warn and go on)")
    p.add_argument("--device", type=int, default=0, help="GPU to run on (default: %(default)d)")
    p.add_argument("--gpus", type=int, default=None,
                   help="GPUs to run on, one process (rank) each, devices 0..N-1 (default: one GPU, --device)")
    p.add_argument("--batch-clusters", type=int, default=BATCH_CLUSTERS,
                   help="gene clusters per GPU batch (default: %(default)d)")
    p.add_argument("-v", action="count", default=0, help="more log output (-v: debug)")
    p.add_argument("--version", action="version", version="%(prog)s " + __version__)
    return p.parse_args(argv)


def set_logging(v):
    """log records to stderr: info by default, debug from -v on"""
    logger.setLevel(logging.DEBUG)
    for h in list(logger.handlers):
        if getattr(h, "_panfeed_cli", False):
            logger.removeHandler(h)
    ch = logging.StreamHandler(sys.stderr)
    ch.setLevel(logging.INFO if v == 0 else logging.DEBUG)
    ch.setFormatter(logging.Formatter("%(asctime)s - %(name)s - %(levelname)s - %(message)s", "%H:%M:%S"))
    ch._panfeed_cli = True
    logger.addHandler(ch)


def read_names(path):
    """one name per line, only the trailing newline stripped (input.py:198-211)"""
    with open(path) as fh:
        return {line.rstrip("\n") for line in fh}


def is_hashed_pattern(text):
    """whether `text` is a hashed_pattern as the files print it: the 24 base64 characters of a 16-byte digest"""
    import binascii
    if len(text) != 24:
        return False
    try:
        d = binascii.a2b_base64(text)
    except (binascii.Error, ValueError):
        return False
    return len(d) == 16 and binascii.b2a_base64(d)[:24].decode() == text


def passing_hashes(values, source):
    """the hashed_pattern values among `values` (strings), in order and once each; a blank one is skipped, any other that
    is no such digest matches nothing: their number is logged once, as a warning"""
    good, bad = {}, 0
    for v in values:
        v = v.rstrip("\r\n")
        if not v.strip():
            continue
        if is_hashed_pattern(v):
            good[v] = None
        else:
            bad += 1
    if bad:
        logger.warning(f"{bad} entr{'y' if bad == 1 else 'ies'} of {source} {'is' if bad == 1 else 'are'} not a "
                       "hashed_pattern (24 base64 characters of a 16-byte digest) and match nothing")
    return list(good)


def associations_hashes(path, threshold, column, device):
    """the passing hashes of an associations table, as the downstream tools take them (downstream._associations: the same
    device pass, the same fallbacks; a missing column ends the command with status 1 and the tools' message)"""
    import argparse
    from . import downstream
    ns = argparse.Namespace(associations=path, threshold=threshold, column=column, output=None, device=device,
                            host_gunzip=False, host_associations=False)
    return downstream._associations(ns, index_name="hashed_pattern")[1]


def main(argv=None, run=None, launch=None, rank_entry=None, associations=None):
    """the panfeed command; returns the exit status.  run: what does the work on one GPU (default pipeline.run_files);
    launch: what starts the ranks of `--gpus N` (default rank.launch); rank_entry: what this process does as one rank of
    a launcher's world (default rank.run_rank); associations: what reads the passing hashes of --passing-associations
    (default associations_hashes).  Tests pass their own."""
    from . import rank as rank_mod
    args = get_options(argv)
    set_logging(args.v)
    k = args.kmer_length
    if args.downstream_start_codon and args.upstream + args.downstream < k:
        logger.warning("The sequence around the start codon (--upstream + --downstream) is shorter than the k-mer "
                       "length: lower -k or widen the flanks")
        return 1
    if args.maf > 0.5:
        logger.warning("--maf must not be above 0.5")
        return 1
    if not 1 <= k <= PF_MAX_K:
        logger.error(f"-k {k} is outside 1..{PF_MAX_K} (PF_MAX_K): the GPU's k-mer keys hold at most {PF_MAX_K} bases")
        return 2
    if args.cores != 1 or args.queue_limit != 3:
        logger.debug(f"--cores {args.cores} / --queue-limit {args.queue_limit}: no effect, the GPU does the workers' part")
    if args.batch_clusters < 1:
        logger.error("--batch-clusters must be at least 1")
        return 2
    if args.gpu_compress_clusters and not args.multiple_files:
        logger.error("--gpu-compress-clusters is for the per-cluster files of --multiple-files; --gpu-compress compresses the "
                     "one set of files on the GPU")
        return 2
    if args.gpu_compress_level is not None and not (args.gpu_compress or args.gpu_compress_clusters):
        logger.error("--gpu-compress-level sets the effort of the GPU's encoder: give --gpu-compress or "
                     "--gpu-compress-clusters with it")
        return 2
    if args.bgzf:
        if not args.gpu_compress:
            logger.error("--bgzf frames the members --gpu-compress makes: give --gpu-compress with it")
            return 2
        if args.multiple_files or rank_mod.launched() or (args.gpus is not None and args.gpus != 1):
            logger.error("--bgzf is for the three files of a run on one GPU: --multiple-files, --gpus N and a launched rank "
                         "are deliberately out of its scope; nothing was run")
            return 2
    if args.passing_hashes is not None and args.passing_associations is not None:
        logger.error("--passing-hashes and --passing-associations both name the passing patterns: give one of them")
        return 2
    if args.passing_associations is None and (args.passing_threshold is not None or args.passing_column is not None):
        logger.error("--passing-threshold and --passing-column belong to --passing-associations: give it with them")
        return 2
    passing_on = args.passing_hashes is not None or args.passing_associations is not None
    if passing_on and (rank_mod.launched() or (args.gpus is not None and args.gpus != 1)):
        logger.error("--passing-hashes / --passing-associations filter the kmers.tsv of a run on one GPU: --gpus N and a "
                     "launched rank are deliberately out of their scope; nothing was run")
        return 2
    if args.targets is not None:
        logger.debug(f"Reading target strains ({args.targets})")
        targets = read_names(args.targets)
    else:
        logger.warning("No target strains given: kmers.tsv will hold its header only")
        targets = set()
    genes = None
    if args.genes is not None:
        logger.debug(f"Reading gene clusters ({args.genes})")
        genes = read_names(args.genes)
    as_rank = rank_mod.launched()         # (rank 0 creates the directory: the ranks look together, in run_files_sharded)
    if os.path.exists(args.output) and not as_rank:
        logger.error(f"Output directory {args.output} exists: remove it or choose another")
        return 1
    many = as_rank or (args.gpus is not None and args.gpus != 1)
    if args.gpus is not None and args.gpus < 1:
        logger.error("--gpus must be at least 1")
        return 2
    if many and args.device != 0 and not rank_mod.shared_gpu():
        logger.error("--device cannot be combined with a run on several GPUs: rank r runs on GPU r")
        return 2
    if many and not as_rank and not rank_mod.shared_gpu():
        import torch                      # (counting the devices does not initialise the GPU)
        ndev = torch.cuda.device_count()
        if ndev < args.gpus:
            logger.error(f"--gpus {args.gpus}: {ndev} device{'s' if ndev != 1 else ''} on this machine -- one rank per GPU; "
                         "nothing was run (PANFEED_SHARED_GPU=1 rehearses the control flow on one GPU)")
            return 2
    more = {}
    if args.gpu_compress:
        more["device_gzip"] = True
        if args.multiple_files:
            logger.info("--gpu-compress with --multiple-files: the per-cluster files are compressed on the host; "
                        "--gpu-compress-clusters compresses them on the GPU")
    if args.gpu_compress_clusters:
        more["device_gzip_clusters"] = True
    if args.bgzf:
        more["bgzf"] = True
    if args.gpu_compress_level is not None:        # (not given: the default of run_files and run_files_sharded, 1)
        more["device_gzip_level"] = args.gpu_compress_level
    if passing_on:
        if args.passing_hashes is not None:
            logger.debug(f"Reading passing hashes ({args.passing_hashes})")
            with open(args.passing_hashes) as fh:
                more["passing_hashes"] = passing_hashes(fh, args.passing_hashes)
        else:
            try:
                found = (associations or associations_hashes)(
                    args.passing_associations, 1 if args.passing_threshold is None else args.passing_threshold,
                    "lrt-pvalue" if args.passing_column is None else args.passing_column, args.device)
            except SystemExit as e:        # (the tools' way out of a missing column: their message has been logged)
                return e.code if isinstance(e.code, int) else 1
            more["passing_hashes"] = passing_hashes(found, args.passing_associations)
        if not targets:
            logger.info("No target strains: the passing patterns have no kmers.tsv rows to choose among")
        else:
            logger.info(f"kmers.tsv will hold the rows of {len(more['passing_hashes'])} passing patterns only")
    from ._lib import PanfeedHipError
    from .engine import gzip_modes
    compress = gzip_modes(args.compress, args.gpu_compress, args.multiple_files, args.gpu_compress_clusters)[0]
    if many:
        options = dict(fastadir=args.fasta, klength=k, canon=not args.non_canonical, consider_missing=args.consider_missing,
                       patfilt=not args.no_filter, maf=args.maf, upstream=args.upstream, downstream=args.downstream,
                       downstream_start_codon=args.downstream_start_codon, targets=tuple(sorted(targets)),
                       genes=sorted(genes) if genes is not None else None, compress=compress,
                       multiple_files=args.multiple_files, batch_clusters=args.batch_clusters, gpu=args.device,
                       raise_missing=args.stop_on_missing, **more)
        if not as_rank:
            logger.info(f"Extracting k-mers on {args.gpus} GPUs" +
                        (" (PANFEED_SHARED_GPU=1: a rehearsal on one)" if rank_mod.shared_gpu() else ""))
            return (launch or rank_mod.launch)(args.gpus, args.presence_absence, args.gff, args.output, verbose=args.v,
                                               **options)
        logger.info(f"Extracting k-mers as rank {os.environ['RANK']} of {os.environ['WORLD_SIZE']}")
        try:
            stats = (rank_entry or rank_mod.run_rank)(args.presence_absence, args.gff, args.output, **options)
        except (PanfeedHipError, FileExistsError, RuntimeError) as e:
            logger.error(str(e))
            return 1
        rank_mod.report(stats or {}, args.output)
        return 0
    if run is None:
        from .pipeline import run_files as run
    logger.info("Extracting k-mers")
    try:
        stats = run(args.presence_absence, args.gff, args.output, fastadir=args.fasta, klength=k,
                    canon=not args.non_canonical, consider_missing=args.consider_missing, patfilt=not args.no_filter,
                    maf=args.maf, upstream=args.upstream, downstream=args.downstream,
                    downstream_start_codon=args.downstream_start_codon, targets=tuple(sorted(targets)),
                    genes=sorted(genes) if genes is not None else None, compress=compress,
                    multiple_files=args.multiple_files, batch_clusters=args.batch_clusters, device=args.device,
                    raise_missing=args.stop_on_missing, **more)
    except PanfeedHipError as e:          # the reader's message under --stop-on-missing, or the library's error
        logger.error(str(e))
        return 1
    stats = stats or {}
    for line in (stats.get("log") or "").splitlines():
        logger.warning(line)
    logger.info(f"{stats.get('clusters', 0)} gene clusters, {stats.get('instances', 0)} k-mer instances, "
                f"{stats.get('patterns', 0)} patterns written to {args.output}" +
                (f"; {stats.get('kmers_rows_kept', 0)} of {stats.get('kmers_rows_considered', 0)} kmers.tsv rows kept "
                 "(passing patterns only)" if passing_on else ""))
    return 0
