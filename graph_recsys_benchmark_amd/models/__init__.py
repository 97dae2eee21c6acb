from .base import GraphRecsysModel, MFRecsysModel, PEABaseChannel, PEABaseRecsysModel
from .peagat import PEAGATChannel, PEAGATRecsysModel
from .peagcn import PEAGCNChannel, PEAGCNRecsysModel
from .peasage import PEASageChannel, PEASageRecsysModel
from .kgat import KGATRecsysModel
from .kgcn import KGCNRecsysModel
from .ngcf import NGCFRecsysModel
from .metapath2vec import MetaPath2Vec
from .walk import WalkBasedRecsysModel
from .herec import HeRecRecsysModel
from .cfkg import CFKGRecsysModel
from .nfm import NFMRecsysModel

__all__ = ['GraphRecsysModel', 'PEABaseChannel', 'PEABaseRecsysModel', 'PEAGATChannel', 'PEAGATRecsysModel',
           'PEAGCNChannel', 'PEAGCNRecsysModel', 'PEASageChannel', 'PEASageRecsysModel', 'KGATRecsysModel', 'KGCNRecsysModel',
           'NGCFRecsysModel', 'MetaPath2Vec', 'WalkBasedRecsysModel', 'HeRecRecsysModel', 'CFKGRecsysModel',
           'MFRecsysModel', 'NFMRecsysModel']
