"""Output-task layout of the four heads and the label algebra the VCF decode needs.

Counterpart of /root/reference/clair/task/{main,gt21,genotype,variant_length}.py: the inference side, and the label
encoders `evaluate` scores a checkpoint against (training itself is out of scope):

  head sizes 21 / 3 / 33 / 33 and their slices in a packed 90-vector   task/main.py:10-29
  the 21 genotype labels and their indices                              task/gt21.py:3-50
  genotype classes 0/0, 1/1, 0/1, 1/2                                   task/genotype.py:3-10
  indel length range -16..+16, index offset 16                          task/variant_length.py:6-12
  gt21 label of a (REF, ALT, genotype) triple                           task/gt21.py:60-110
  true labels of a truth row / of a reference site                      task/main.py:36-81
"""

GT21_LABELS = ("AA", "AC", "AG", "AT", "CC", "CG", "CT", "GG", "GT", "TT",
               "DelDel", "ADel", "CDel", "GDel", "TDel",
               "InsIns", "AIns", "CIns", "GIns", "TIns", "InsDel")
GT21_INDEX = {label: i for i, label in enumerate(GT21_LABELS)}

HOMO_SNP = ("AA", "CC", "GG", "TT")                      # task/gt21.py:112-113
HETERO_SNP = ("AC", "AG", "AT", "CG", "CT", "GT")        # task/gt21.py:115-116
HOMO_SNP_IDX = tuple(GT21_INDEX[s] for s in HOMO_SNP)
HETERO_SNP_IDX = tuple(GT21_INDEX[s] for s in HETERO_SNP)
INS_BASE_IDX = tuple(GT21_INDEX[b + "Ins"] for b in "ACGT")
DEL_BASE_IDX = tuple(GT21_INDEX[b + "Del"] for b in "ACGT")
IDX_INSINS, IDX_DELDEL, IDX_INSDEL = GT21_INDEX["InsIns"], GT21_INDEX["DelDel"], GT21_INDEX["InsDel"]

GENOTYPE_STRINGS = ("0/0", "1/1", "0/1", "1/2")          # task/genotype.py:3
HOMO_REFERENCE, HOMO_VARIANT, HETERO_VARIANT, HETERO_VARIANT_MULTI = 0, 1, 2, 3

LENGTH_OFFSET = 16                                        # task/variant_length.py:6
LENGTH_MAX = 16
N_LENGTH = 2 * LENGTH_OFFSET + 1

SLICES = {"gt21": (0, 21), "genotype": (21, 24), "len1": (24, 57), "len2": (57, 90)}

# shared/utils.py:19-29
IUPAC_TO_NUM = dict(zip("ACGTURYSWKMBDHVN", (0, 1, 2, 3, 3, 0, 1, 1, 0, 2, 0, 1, 0, 0, 0, 0)))
IUPAC_TO_ACGT = dict(zip("ACGTURYSWKMBDHVN", "ACGTTACCAGACAAAA"))
BASIC_BASES = frozenset("ACGTU")


def _allele_kind(ref, alt):
    """task/gt21.py:60-65 -- how one allele differs from REF: 'Del', 'Ins' or its first base."""
    if len(ref) > len(alt):
        return "Del"
    if len(ref) < len(alt):
        return "Ins"
    return alt[0]


def gt21_index_of_call(ref, alt, g1, g2):
    """Index of the gt21 class a VCF call (REF, ALT string, genotype digits) belongs to.

    Follows task/gt21.py:68-110: a single ALT is paired with REF when either genotype digit
    is 0, else with itself; two base alleles sort alphabetically; base+indel gives e.g. 'AIns';
    equal indel kinds give 'InsIns'/'DelDel'; mixed gives 'InsDel'.
    """
    alts = alt.split(",")
    if len(alts) == 1:
        alts = [ref if (g1 == 0 or g2 == 0) else alts[0]] + alts
    a, b = _allele_kind(ref, alts[0]), _allele_kind(ref, alts[1])
    if len(a) == 1 and len(b) == 1:
        label = a + b if a <= b else b + a
    elif len(a) == 1 or len(b) == 1:
        label = (a + b) if len(a) == 1 else (b + a)
    elif a == b:
        label = a + b
    else:
        label = "InsDel"
    return GT21_INDEX[label]


def genotype_class_of(g1, g2):
    """task/genotype.py:19-33: class index used by the genotype head (1/2 folds into 0/1)."""
    if g1 == 0 and g2 == 0:
        return HOMO_REFERENCE
    if g1 == g2:
        return HOMO_VARIANT
    return HETERO_VARIANT


def labels_from_reference(base):
    """task/main.py:36-48 -- true indices (gt21, genotype, len1, len2) of a site without a truth variant: homozygous `base`."""
    return GT21_INDEX[base + base], HOMO_REFERENCE, LENGTH_OFFSET, LENGTH_OFFSET


def labels_from_vcf_columns(columns):
    """task/main.py:51-81 -- true indices (gt21, genotype, len1, len2) of one row `ctg pos ref alt g1 g2` of a truth-variant file
    (clair_amd.get_truth).  A single ALT is paired with REF when a genotype digit is 0, else with itself; 1/2 folds into the
    heterozygous class (task/genotype.py:20-33); the two allele lengths are clamped to -16..+16 and put in ascending order."""
    ref, alt = columns[2], columns[3]
    g1, g2 = int(columns[4]), int(columns[5])
    alts = alt.split(",")
    if len(alts) == 1:
        alts = [ref if (g1 == 0 or g2 == 0) else alts[0]] + alts
    lengths = sorted(max(min(len(a) - len(ref), LENGTH_MAX), -LENGTH_MAX) for a in alts)
    return gt21_index_of_call(ref, alt, g1, g2), genotype_class_of(g1, g2), lengths[0] + LENGTH_OFFSET, lengths[1] + LENGTH_OFFSET


def one_hot_labels(indices):
    """The reference's 90-element label vector (task/main.py:48, :81) from the four true indices."""
    vec = [0] * SLICES["len2"][1]
    for (start, _), index in zip((SLICES[k] for k in ("gt21", "genotype", "len1", "len2")), indices):
        vec[start + index] = 1
    return vec
