from _inert import Inert
def __getattr__(name):
    return Inert("geomloss." + name)
